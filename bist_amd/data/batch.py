"""The ``Batch`` contract the hot path consumes (reference: data/dataset.py:59-131).

Only the fields and masks that ``MTN.forward`` / the generators read are built here; loading
AVSD json/.npy files is out of scope.  Unlike the reference's Batch the
masks can be derived on the device: ``temporal_mask`` comes from a HIP reduction over the
features (``ops.temporal_mask``) instead of a host-side ``fts.sum(2).sum(-1) != 0``.
"""
from __future__ import annotations

from typing import Optional

import torch

PAD = 1  # '<blank>' (data/data_handler.py:23; collate pads with 1, dataset.py:184-193)


def subsequent_mask(size: int, device=None) -> torch.Tensor:
    """[1,size,size] bool, True where a position may be attended (data/data_utils.py:14-18)."""
    m = torch.ones(1, size, size, dtype=torch.bool, device=device).tril_()
    m._bist_causal = size          # content tag: consumers may cache what they derive from a pure causal mask by its size alone
    return m


class Batch:
    """Same attribute names as the reference Batch (dataset.py:59-99).

    query/his/cap/trg/trg_y: int64 [B, L*]; fts: float [B,T,S,C] (f32 or bf16); audio_fts: as the reference passes it -- None, or a
    list holding one [B,Ta,Da] array (numpy or tensor; a bare tensor is accepted too) -- dataset.py:60, 83-87.
    """

    def __init__(self, query, his, fts, cap, trg, trg_y=None, pad: int = PAD, vids=None, qa_ids=None, audio_fts=None):
        self.vids, self.qa_ids = vids, qa_ids
        self.query, self.his, self.cap, self.trg, self.trg_y = query, his, cap, trg, trg_y
        self.fts = fts
        self.query_mask = (query != pad).unsqueeze(-2)              # dataset.py:66
        self.query_mask2 = torch.cat([self.query_mask, self.query_mask], dim=0)   # the same mask for the stacked (t2s, s2t) batch of a reasoning layer
        self.his_mask = (his != pad).unsqueeze(-2)                  # dataset.py:67
        self.cap_mask = (cap != pad).unsqueeze(-2) if cap is not None else None   # dataset.py:92
        self.temporal_mask: Optional[torch.Tensor] = None           # dataset.py:79 (device-side, see below)
        self.trg_mask = self.make_std_mask(trg, pad)                # dataset.py:96
        self.trg_mean_mask = (trg_y != pad) if trg_y is not None else None
        self.ntokens = (trg_y != pad).sum() if trg_y is not None else None   # dataset.py:98
        self.qntokens = (query != pad).sum()                        # dataset.py:99
        self.audio_fts = _audio_tensor(audio_fts)                   # dataset.py:83-86
        self.audio_mask = None
        if fts is not None:
            self._derive_temporal_mask()
        if self.audio_fts is not None:
            self._derive_audio_mask()

    def _derive_temporal_mask(self):
        if self.fts.is_cuda:
            from .. import ops
            self.temporal_mask = ops.temporal_mask(self.fts)
        else:   # host-side batches (before move_to_cuda) follow the reference expression literally
            self.temporal_mask = (self.fts.sum(2).sum(-1) != 0).unsqueeze(-2)

    def _derive_audio_mask(self):
        """audio_mask = (audio_fts.sum(-1) != 0).unsqueeze(-2) (dataset.py:87): the SUM of a row, so a row whose entries cancel is masked."""
        if self.audio_fts.is_cuda:
            from .. import ops
            self.audio_mask = ops.audio_mask(self.audio_fts)
        else:
            self.audio_mask = (self.audio_fts.sum(-1) != 0).unsqueeze(-2)

    @staticmethod
    def make_std_mask(tgt, pad):
        """pad mask AND causal mask -> [B,Lt,Lt] (dataset.py:101-105)."""
        return (tgt != pad).unsqueeze(-2) & subsequent_mask(tgt.size(-1), tgt.device)

    def move_to_cuda(self):
        """dataset.py:107-127."""
        for name in ("query", "his", "cap", "trg", "trg_y", "query_mask", "query_mask2", "his_mask", "cap_mask", "trg_mask",
                     "trg_mean_mask", "fts", "temporal_mask", "audio_fts", "audio_mask"):
            v = getattr(self, name)
            if v is not None:
                setattr(self, name, v.to("cuda", non_blocking=True))
        return self


def _audio_tensor(audio_fts):
    """The reference's audio argument -- None, an empty list, or a list holding one [B,Ta,Da] array (dataset.py:85-86) -- as a tensor."""
    if audio_fts is None:
        return None
    if isinstance(audio_fts, (list, tuple)):
        if len(audio_fts) == 0:
            return None
        audio_fts = audio_fts[0]
    if not torch.is_tensor(audio_fts):
        audio_fts = torch.from_numpy(audio_fts).float()
    if audio_fts.dim() != 3:
        raise ValueError("audio_fts must be [B, Ta, Da]")
    return audio_fts


_DERIVED = ("query_mask", "query_mask2", "his_mask", "cap_mask", "trg_mask", "trg_mean_mask", "temporal_mask")


class SourceBatch(Batch):
    """A Batch whose derived fields -- the masks and ``temporal_mask`` -- are built on FIRST ACCESS only.  What the class-mode Trainer
    reads of a batch is its ids, features and token counts: its staging launch (bist_stage_train_batch) derives every mask again, at
    the class lengths.  A batch handed to it this way costs two token counts instead of ten mask launches and a pass of
    bist_temporal_mask over the features, so a fed class step reads the features once.  Any other consumer sees a complete Batch."""

    def __init__(self, query, his, fts, cap, trg, trg_y=None, pad: int = PAD, vids=None, qa_ids=None, audio_fts=None):
        self.vids, self.qa_ids = vids, qa_ids
        self.query, self.his, self.cap, self.trg, self.trg_y = query, his, cap, trg, trg_y
        self.fts = fts
        self.pad = pad
        self.ntokens = (trg_y != pad).sum() if trg_y is not None else None   # dataset.py:98
        self.qntokens = (query != pad).sum()                                  # dataset.py:99
        self.audio_fts = _audio_tensor(audio_fts)
        if self.audio_fts is None:
            self.audio_mask = None                                            # (with audio: derived on first access, like the other masks)

    def __getattr__(self, name):
        # (called only for attributes not set yet: the derived fields, all at once, from the fields as they are now)
        if (name not in _DERIVED and name != "audio_mask") or "query" not in self.__dict__:
            raise AttributeError(name)
        full = Batch(self.query, self.his, self.fts, self.cap, self.trg, self.trg_y, pad=self.pad, audio_fts=self.audio_fts)
        for f in _DERIVED + (("audio_mask",) if self.audio_fts is not None else ()):
            self.__dict__.setdefault(f, getattr(full, f))
        return self.__dict__[name]
