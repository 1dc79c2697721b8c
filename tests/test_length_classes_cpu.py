"""Length classes of ragged training batches (bist_amd.data.classes): the ladder mapping, key stability, ``fixed()``, lengths beyond the
last rung, and the rule that a class geometry selects the same kernel forms as every exact geometry mapped onto it (the fused stage-1
envelope probes are host functions of the library).  No GPU."""
import ctypes
import os
import subprocess

import pytest
import torch

from bist_amd.data.classes import DEFAULT_RUNGS, FIELDS, LengthClasses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _B:
    def __init__(self, B=4, Lq=7, Lh=9, Lc=6, Lt=6, T=6, S=9, C=64, cap=True, dtype=torch.float32):
        self.query = torch.zeros(B, Lq, dtype=torch.int64)
        self.his = torch.zeros(B, Lh, dtype=torch.int64)
        self.cap = torch.zeros(B, Lc, dtype=torch.int64) if cap else None
        self.trg = torch.zeros(B, Lt, dtype=torch.int64)
        self.trg_y = torch.zeros(B, Lt, dtype=torch.int64)
        self.fts = torch.zeros(B, T, S, C, dtype=dtype)


def test_ladder_maps_to_the_smallest_rung_at_least_as_long():
    lc = LengthClasses()
    for f in FIELDS:
        rungs = DEFAULT_RUNGS[f]
        prev = 0
        for r in rungs:
            for L in range(prev + 1, r + 1):
                assert lc.round(f, L) == r, (f, L)
            prev = r
    assert lc.shape(_B(Lq=20, Lh=60, Lc=25, Lt=20, T=32)) == {"query": 24, "his": 64, "cap": 32, "trg": 24, "frames": 32}


def test_lengths_beyond_the_last_rung_round_up_to_the_step():
    lc = LengthClasses({"query": (8, 16), "his": (32,), "cap": (16,), "trg": (8,), "frames": (32,)},
                       {"query": 16, "his": 64, "cap": 32, "trg": 16, "frames": 32})
    assert lc.round("query", 17) == 32 and lc.round("query", 33) == 48
    assert lc.round("his", 33) == 64 and lc.round("his", 129) == 192
    assert lc.round("frames", 33) == 64
    for L in range(1, 400):
        for f in FIELDS:
            assert lc.round(f, L) >= L
    with pytest.raises(ValueError):
        lc.round("query", 0)


def test_key_is_stable_within_a_class_and_distinguishes_what_shapes_a_graph():
    lc = LengthClasses()
    a, b = lc.key(_B(Lq=17, Lh=40, Lc=20, Lt=9, T=20)), lc.key(_B(Lq=24, Lh=64, Lc=32, Lt=16, T=24))
    assert a == b and hash(a) == hash(b)
    assert lc.key(_B(Lq=25)) != lc.key(_B(Lq=24))                     # another query class
    assert lc.key(_B(B=3)) != lc.key(_B(B=4))                         # B is never padded
    assert lc.key(_B(cap=False)) != lc.key(_B())                      # with / without a caption
    assert lc.key(_B(dtype=torch.bfloat16)) != lc.key(_B())           # feature dtype
    assert lc.key(_B(S=49)) != lc.key(_B())                           # feature row shape
    assert lc.shape(_B(cap=False))["cap"] is None


def test_fixed_is_one_class_for_a_whole_dataset():
    lc = LengthClasses.fixed(query=32, his=128, cap=64, trg=32, frames=32)
    keys = {lc.key(_B(Lq=q, Lh=h, Lc=c, Lt=t, T=T)) for q in (1, 9, 32) for h in (3, 100, 128) for c in (5, 64) for t in (2, 32) for T in (1, 17, 32)}
    assert len(keys) == 1
    assert lc.round("query", 33) == 64 and lc.round("frames", 40) == 64


def test_bad_ladders_are_refused():
    with pytest.raises(ValueError):
        LengthClasses({"query": (16, 8)})
    with pytest.raises(ValueError):
        LengthClasses({"his": (0, 8)})
    with pytest.raises(ValueError):
        LengthClasses(steps={"trg": 0})


def test_default_ladder_keeps_the_kernel_forms_of_every_exact_geometry():
    """Fused stage-1 (inference and training forms, both directions) at the model's head geometry (d=512, h=8, bf16, 7x7 regions) and the
    value-projection owner switch of functional.fused_train_own_v: the same for every exact (query length, frames) and its class."""
    from bist_amd import functional as Fn, ops
    lc = LengthClasses()
    for T in range(1, 200):
        PT = lc.round("frames", T)
        assert Fn.fused_train_own_v(T) == Fn.fused_train_own_v(PT), (T, PT)
        for Lq in range(1, 80):
            PQ = lc.round("query", Lq)
            for dr in (0, 1):
                for probe in (ops.st_stage1_fused_ok, ops.st_stage1_fused_train_ok):
                    assert probe(T, 49, Lq, 512, 8, dr, torch.bfloat16) == probe(PT, 49, PQ, 512, 8, dr, torch.bfloat16), \
                        (probe.__name__, T, Lq, dr, PT, PQ)
    # the bench geometry stays inside the fused training envelope after padding
    assert all(ops.st_stage1_fused_train_ok(32, 49, 24, 512, 8, dr, torch.bfloat16) for dr in (0, 1))


def test_stage_descriptor_layout_matches_the_header(tmp_path):
    from bist_amd import _lib
    fields = ["src", "dst", "query_mask", "temporal_mask", "d_qntokens", "fts", "d_fts", "src_ld", "row_elems", "pad", "src_len",
              "dst_len", "B", "PT", "out_dtype", "reserved_"]
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "bist_hip.h"', "int main(void) {",
           '  printf("size %zu\\n", sizeof(BistTrainStage));']
    src += [f'  printf("{f} %zu\\n", offsetof(BistTrainStage, {f}));' for f in fields]
    src += ["  return 0;", "}"]
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    seen = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert ctypes.sizeof(_lib.BistTrainStage) == int(seen["size"])
    for f in fields:
        assert getattr(_lib.BistTrainStage, f).offset == int(seen[f]), f


def test_trainer_and_feeder_take_length_classes():
    import inspect
    from bist_amd.data.feeder import DeviceFeeder
    from bist_amd.train import Trainer
    assert "length_classes" in inspect.signature(Trainer.__init__).parameters
    assert "max_graphs" in inspect.signature(Trainer.__init__).parameters
    assert "length_classes" in inspect.signature(DeviceFeeder.__init__).parameters
    assert hasattr(Trainer, "graph_stats")


def test_source_batch_derives_its_masks_on_first_access_only():
    """What a class-mode feeder yields: ids, features and token counts at once, the masks only when read -- then exactly Batch's."""
    from bist_amd.data.batch import Batch, SourceBatch
    from bist_amd.data.synthetic import synthetic_batch
    b = synthetic_batch(3, T=5, S=2, C=8, Lq=4, Lh=5, Lc=3, Lt=4, vocab=50, device="cpu", dtype=torch.float32)
    s = SourceBatch(b.query, b.his, b.fts, b.cap, b.trg, b.trg_y)
    assert not any(f in s.__dict__ for f in ("query_mask", "his_mask", "trg_mask", "temporal_mask"))
    assert torch.equal(s.ntokens, b.ntokens) and torch.equal(s.qntokens, b.qntokens)
    for f in ("query_mask", "query_mask2", "his_mask", "cap_mask", "trg_mask", "trg_mean_mask", "temporal_mask"):
        assert torch.equal(getattr(s, f), getattr(b, f)), f
    with pytest.raises(AttributeError):
        s.no_such_field
    assert isinstance(s, Batch)
