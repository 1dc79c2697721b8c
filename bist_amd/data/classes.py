"""Length classes of ragged training batches (reference: data/dataset.py:133-195 -- collate_fn pads each batch to its own maxima).

A captured training step replays one fixed geometry.  Real batches come in a new (query, history, caption, answer, frames) geometry
almost every step, so the class-mode ``Trainer`` maps every batch to a LENGTH CLASS -- each varying length rounded up to the next rung of
its ladder -- and replays one captured step per class; ``bist_stage_train_batch`` writes the exact batch into the class-shaped buffers
(ids padded with the pad id, masks derived from them, zero frames appended).  Padding is exact in this model: every attention masks padded
keys, padded targets / queries are excluded from the losses and the token counts, zero frames are excluded by ``temporal_mask``.  Only the
summation order of some reductions can change (rounding level).

Fields: ``query``, ``his``, ``cap``, ``trg`` (trg / trg_y / trg_mask) and ``frames`` (T of ``fts``).  The batch dimension is never padded:
a short last batch is a class of its own.

The default ladder keeps a rule: a class geometry selects the same kernel forms as every exact geometry mapped onto it.
  * fused stage-1 training launch (``bist_st_stage1_fused_train_ok``): Lq <= 32 and, at T <= 32 (two key tiles per group, four groups),
    Lq <= 24 -- hence the query rung 24 -- and frames <= 128 with the tile switches at 32 / 64 frames: frame rungs never cross 32, 64, 128;
  * ``functional.fused_train_own_v``: the value projection changes owner at T >= 64 -- hence the frame rung 63 below 64.
Rungs beyond these switches only trade padded work against the number of graphs (DESIGN.md section 10 measures both).

Batches with audio features (``audio_fts`` [B, Ta, Da]) have a sixth class length, ``audio`` (Ta): ``bist_stage_audio`` writes the exact
rows into the class buffer, appends zero rows and derives ``audio_mask``; a zero row is masked by the reference's own rule
(dataset.py:87).  Its ladder keeps the rule above: the small-attention MFMA backward covers Lk <= 64 keys, so no audio rung straddles 64.
A batch without audio has the five fields above and the same ``lengths()`` / ``shape()`` / ``key()`` as ever.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

FIELDS = ("query", "his", "cap", "trg", "frames")

# rungs per field, and the step that lengths beyond the last rung round up to a multiple of
DEFAULT_RUNGS = {
    "query": (8, 16, 24, 32),
    "his": (32, 64, 96, 128, 192, 256),
    "cap": (16, 32, 48, 64),
    "trg": (8, 16, 24, 32),
    "frames": (8, 16, 24, 32, 48, 63, 64, 96, 128),
}
DEFAULT_STEPS = {"query": 16, "his": 64, "cap": 32, "trg": 16, "frames": 32}
AUDIO = "audio"                              # the sixth field, present only for batches that carry audio features
DEFAULT_AUDIO_RUNGS = (16, 32, 48, 64)       # then multiples of 32: 96, 128, ... (no rung straddles 64)
DEFAULT_AUDIO_STEP = 32


class LengthClasses:
    """A rung ladder per varying length.  ``rungs[f]``: ascending lengths; a length L maps to the smallest rung >= L, or -- beyond the last
    rung -- to the next multiple of ``steps[f]`` (never below L)."""

    def __init__(self, rungs: Optional[Dict[str, Sequence[int]]] = None, steps: Optional[Dict[str, int]] = None):
        rungs = dict(DEFAULT_RUNGS if rungs is None else rungs)
        steps = dict(DEFAULT_STEPS if steps is None else steps)
        self.rungs: Dict[str, Tuple[int, ...]] = {}
        self.steps: Dict[str, int] = {}
        for f in FIELDS + (AUDIO,):
            r = tuple(int(x) for x in rungs.get(f, DEFAULT_AUDIO_RUNGS if f == AUDIO else DEFAULT_RUNGS.get(f)))
            if not r or any(x < 1 for x in r) or any(b <= a for a, b in zip(r, r[1:])):
                raise ValueError(f"LengthClasses: rungs of {f!r} must be ascending positive lengths, got {r}")
            s = int(steps.get(f, DEFAULT_AUDIO_STEP if f == AUDIO else DEFAULT_STEPS.get(f)))
            if s < 1:
                raise ValueError(f"LengthClasses: step of {f!r} must be positive")
            self.rungs[f], self.steps[f] = r, s

    @classmethod
    def fixed(cls, query: int, his: int, cap: int, trg: int, frames: int, audio: Optional[int] = None) -> "LengthClasses":
        """One rung per field: every batch within these lengths replays ONE graph (per batch size); longer ones round up to multiples of it."""
        v = {"query": query, "his": his, "cap": cap, "trg": trg, "frames": frames}
        if audio is not None:
            v[AUDIO] = audio
        return cls({f: (int(n),) for f, n in v.items()}, {f: int(n) for f, n in v.items()})

    def round(self, field: str, length: int) -> int:
        length = int(length)
        if length < 1:
            raise ValueError(f"LengthClasses: {field} length {length} < 1")
        for r in self.rungs[field]:
            if length <= r:
                return r
        s = self.steps[field]
        return max(-(-length // s) * s, length)

    @staticmethod
    def lengths(batch) -> Dict[str, Optional[int]]:
        """The exact lengths of a batch (bist_amd.data.Batch or HostBatch): token tensors [B, L], features [B, T, S, C]."""
        out = {"query": batch.query.shape[-1], "his": batch.his.shape[-1],
               "cap": batch.cap.shape[-1] if getattr(batch, "cap", None) is not None else None,
               "trg": batch.trg.shape[-1], "frames": batch.fts.shape[1]}
        au = getattr(batch, "audio_fts", None)
        if au is not None:
            out[AUDIO] = au.shape[1]          # only with audio: a batch without it has the five fields above and nothing else
        return out

    def shape(self, batch) -> Dict[str, Optional[int]]:
        """The class geometry of a batch: field -> class length (``cap`` None without a caption)."""
        return {f: (None if n is None else self.round(f, n)) for f, n in self.lengths(batch).items()}

    def key(self, batch) -> tuple:
        """Hashable class key: batch size, class lengths, feature row shape and dtypes, whether a caption / answer is present."""
        shp = self.shape(batch)
        fts = batch.fts
        trg_y = getattr(batch, "trg_y", None)
        key = (int(batch.query.shape[0]),) + tuple(shp[f] for f in FIELDS) + (
            tuple(fts.shape[2:]), str(fts.dtype), str(batch.query.dtype), batch.cap is not None, trg_y is not None)
        au = getattr(batch, "audio_fts", None)
        if au is not None:                    # appended only with audio: the class length, the feature width and dtype
            key += (shp[AUDIO], int(au.shape[2]), str(au.dtype))
        return key

    def __repr__(self) -> str:
        return "LengthClasses(%s)" % ", ".join(f"{f}={self.rungs[f]}+{self.steps[f]}k" for f in FIELDS)
