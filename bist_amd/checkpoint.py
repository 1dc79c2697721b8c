"""Trainer checkpoints: the device snapshot of a trainer's optimiser state and the file format built on it --
the counterpart of the reference's ``torch.save`` of the model after validation and of the best one so far (train.py:156-177).

The state of a ``bist_amd.train.Trainer`` between two optimiser steps is the fp32 master weights, the Adam moments ``m`` and ``v``
(three flat device buffers of ``numel`` elements), the device scalars ``hyper[5:8]`` and ``skipped`` of a clipping trainer, and the host
values ``_step``, ``_passes`` and the dropout seed state ``functional._SEED``.  The gradient buffer is not state.  A ``TrainerSnapshot``
holds a copy of all of it: the three buffers on the device (12 bytes per parameter), written by ONE ``bist_state_copy`` launch that
also leaves the 64-bit digests of the bits it copied (include/bist_hip.h has the definition).  ``state_dict()`` turns a snapshot into
CPU data of types ``torch.load(..., weights_only=True)`` accepts; ``validate`` checks such a dictionary against a trainer on the host.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from ._lib import STATE_MAX_SLOTS, check, lib
from .ops import _stream, dtype_code

FORMAT, VERSION = "bist_amd.trainer", 1
# digest slots of a launch: one workgroup per slot -- 1024 chunks of 128 K elements at BASELINE configs[1], every CU holds several (the
# sizing of train.CLIP_SLOTS_BIG).  The digest itself does not depend on the number.
SLOTS = 1024
assert SLOTS <= STATE_MAX_SLOTS
CONFIG_STRICT = ("d_model", "warmup", "factor", "betas", "eps")      # load_state_dict(strict=True) compares these
_DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16}
_MASK = (1 << 64) - 1


def state_copy(src, dst, work: Optional[torch.Tensor], digests: torch.Tensor, max_blocks: int = 0) -> None:
    """One bist_state_copy on the current stream.  src, dst: (p, m, v) fp32 device tensors of one length, dst None: digest only;
    work: the compute-dtype copy refreshed from src's weights, or None; digests: int64 [3, nslots]."""
    n = src[0].numel()
    assert all(t.numel() == n and t.dtype == torch.float32 and t.is_contiguous() for t in src)
    assert dst is None or all(t.numel() == n and t.dtype == torch.float32 and t.is_contiguous() for t in dst)
    assert digests.dtype == torch.int64 and digests.dim() == 2 and digests.shape[0] == 3 and digests.is_contiguous()
    d = [None] * 3 if dst is None else [t.data_ptr() for t in dst]
    check(lib.bist_state_copy(src[0].data_ptr(), src[1].data_ptr(), src[2].data_ptr(), d[0], d[1], d[2],
                              None if work is None else work.data_ptr(), 0 if work is None else dtype_code(work.dtype), n,
                              digests.data_ptr(), digests.shape[1], max_blocks, _stream()), "bist_state_copy")


def digest_totals(digests: torch.Tensor) -> Dict[str, int]:
    """Synchronises: the per-slot digests [3, nslots] -> {"master", "m", "v"}, each the sum modulo 2^64 of its slots."""
    rows = digests.cpu().numpy().view(np.uint64)
    return {k: int(np.add.reduce(rows[i], dtype=np.uint64)) & _MASK for i, k in enumerate(("master", "m", "v"))}


class TrainerSnapshot:
    """The optimiser state of a trainer as it was between two steps: three fp32 device buffers, the per-slot digests of what was
    copied into them, the device scalars, and the host counters read when the snapshot was taken.  Made by ``Trainer.snapshot()``,
    consumed by ``Trainer.restore()``; ``state_dict()`` is its host form."""

    def __init__(self, numel: int, device, clip: bool):
        self.numel = int(numel)
        self.master = torch.empty(numel, device=device, dtype=torch.float32)
        self.m = torch.empty(numel, device=device, dtype=torch.float32)
        self.v = torch.empty(numel, device=device, dtype=torch.float32)
        self.digests = torch.zeros(3, SLOTS, device=device, dtype=torch.int64)
        self.hyper = torch.zeros(8, device=device, dtype=torch.float32)
        self.skipped = torch.zeros(1, device=device, dtype=torch.int64) if clip else None
        self.step = self.passes = 0
        self.seed = (0, 0)
        self.layout: Dict[str, object] = {}
        self.config: Dict[str, object] = {}
        self.event = None                  # recorded behind the launches that fill the snapshot

    @property
    def world(self) -> int:
        return int(self.config.get("world", 1))

    def tensors(self):
        return (self.master, self.m, self.v)

    def state_dict(self) -> Dict[str, object]:
        """Waits for the snapshot's launches, then returns CPU data only (tensors, strings, numbers, lists, dictionaries)."""
        if self.event is not None:
            self.event.synchronize()
        return {"format": FORMAT, "version": VERSION,
                "layout": {k: (list(v) if isinstance(v, (list, tuple)) else v) for k, v in self.layout.items()},
                "config": dict(self.config),
                "counters": {"step": int(self.step), "passes": int(self.passes),
                             "skipped": int(self.skipped.item()) if self.skipped is not None else 0},
                "dropout": {"seed": int(self.seed[0]), "draws": int(self.seed[1])},
                "hyper": self.hyper.cpu(),
                "master": self.master.cpu(), "m": self.m.cpu(), "v": self.v.cpu(),
                "digest": digest_totals(self.digests)}


def describe(trainer) -> Tuple[Dict[str, object], Dict[str, object]]:
    """The ``layout`` and ``config`` entries of a checkpoint of `trainer`."""
    lay = trainer._layout
    layout = {"numel": int(trainer.numel), "n32": int(trainer.n32), "names": [e[0] for e in lay], "offsets": [int(e[1]) for e in lay],
              "shapes": [list(e[3]) for e in lay]}
    config = {"compute_dtype": str(trainer.compute_dtype).replace("torch.", ""), "d_model": int(trainer.args.d_model),
              "warmup": float(trainer.warmup), "factor": float(trainer.factor), "betas": [float(b) for b in trainer.betas],
              "eps": float(trainer.eps), "accumulate": bool(trainer.accumulate),
              "max_grad_norm": None if trainer.max_grad_norm is None else float(trainer.max_grad_norm),
              "deterministic": bool(trainer.deterministic), "world": int(trainer.world)}
    return layout, config


_KEYS = {"": ("format", "version", "layout", "config", "counters", "dropout", "hyper", "master", "m", "v", "digest"),
         "layout": ("numel", "n32", "names", "offsets", "shapes"),
         "config": ("compute_dtype", "d_model", "warmup", "factor", "betas", "eps", "accumulate", "max_grad_norm", "deterministic", "world"),
         "counters": ("step", "passes", "skipped"),
         "dropout": ("seed", "draws"),
         "digest": ("master", "m", "v")}


def validate(sd, trainer, strict: bool = True) -> None:
    """Host-side check of a checkpoint dictionary against `trainer`: raises ValueError naming the field; launches nothing."""
    if not isinstance(sd, dict):
        raise ValueError("checkpoint: expected a dictionary, got %s" % type(sd).__name__)
    if sd.get("format") != FORMAT:
        raise ValueError("checkpoint: format %r, expected %r" % (sd.get("format"), FORMAT))
    if sd.get("version") != VERSION:
        raise ValueError("checkpoint: version %r, this build reads version %d" % (sd.get("version"), VERSION))
    for group, keys in _KEYS.items():
        part = sd if group == "" else sd[group]
        if not isinstance(part, dict):
            raise ValueError("checkpoint: %s is not a dictionary" % group)
        for k in keys:
            if k not in part:
                raise ValueError("checkpoint: missing key %s" % (k if group == "" else group + "." + k))
    layout, config = describe(trainer)
    got = sd["layout"]
    for k in ("numel", "n32"):
        if got[k] != layout[k]:
            raise ValueError("checkpoint: layout.%s is %r, the trainer's is %r" % (k, got[k], layout[k]))
    if len(got["names"]) != len(layout["names"]) or len(got["offsets"]) != len(got["names"]) or len(got["shapes"]) != len(got["names"]):
        raise ValueError("checkpoint: layout.names has %d parameters, the trainer %d" % (len(got["names"]), len(layout["names"])))
    for i, name in enumerate(layout["names"]):
        if got["names"][i] != name:
            raise ValueError("checkpoint: layout.names[%d] is %r, the trainer's is %r" % (i, got["names"][i], name))
        if got["offsets"][i] != layout["offsets"][i]:
            raise ValueError("checkpoint: layout.offsets[%d] (%s) is %r, the trainer's is %r" % (i, name, got["offsets"][i], layout["offsets"][i]))
        if list(got["shapes"][i]) != layout["shapes"][i]:
            raise ValueError("checkpoint: layout.shapes[%d] (%s) is %r, the trainer's is %r" % (i, name, list(got["shapes"][i]), layout["shapes"][i]))
    for k in ("master", "m", "v"):
        t = sd[k]
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 1 or t.numel() != layout["numel"]:
            raise ValueError("checkpoint: %s must be a float32 tensor of %d elements, got %s" % (
                k, layout["numel"], "%s[%s]" % (t.dtype, ", ".join(map(str, t.shape))) if isinstance(t, torch.Tensor) else type(t).__name__))
    h = sd["hyper"]
    if not isinstance(h, torch.Tensor) or h.dtype != torch.float32 or tuple(h.shape) != (8,):
        raise ValueError("checkpoint: hyper must be a float32 tensor of 8 elements")
    if sd["config"]["compute_dtype"] not in _DTYPES:
        raise ValueError("checkpoint: config.compute_dtype %r is not one of %s" % (sd["config"]["compute_dtype"], sorted(_DTYPES)))
    for group, keys in (("counters", _KEYS["counters"]), ("dropout", _KEYS["dropout"]), ("digest", _KEYS["digest"])):
        for k in keys:
            x = sd[group][k]
            if isinstance(x, bool) or not isinstance(x, int) or x < 0:
                raise ValueError("checkpoint: %s.%s must be a non-negative integer, got %r" % (group, k, x))
    if strict:
        for k in CONFIG_STRICT:
            a, b = sd["config"][k], config[k]
            if (list(a) if isinstance(a, (list, tuple)) else a) != b:
                raise ValueError("checkpoint: config.%s is %r, the trainer's is %r (strict=False keeps the trainer's)" % (k, a, b))


def upload(sd, trainer) -> TrainerSnapshot:
    """A validated checkpoint dictionary as a device snapshot on `trainer`'s device (12 bytes per parameter)."""
    dev = trainer.master.device
    snap = TrainerSnapshot(trainer.numel, dev, clip=True)
    snap.master.copy_(sd["master"])
    snap.m.copy_(sd["m"])
    snap.v.copy_(sd["v"])
    snap.hyper.copy_(sd["hyper"])
    snap.skipped.fill_(int(sd["counters"]["skipped"]))
    snap.step, snap.passes = int(sd["counters"]["step"]), int(sd["counters"]["passes"])
    snap.seed = (int(sd["dropout"]["seed"]), int(sd["dropout"]["draws"]))
    snap.layout, snap.config = dict(sd["layout"]), dict(sd["config"])
    return snap
