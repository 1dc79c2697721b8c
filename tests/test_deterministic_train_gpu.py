"""Trainer(deterministic=True): bit-reproducible training steps, at the small model sizes of
tests/test_ragged_train_gpu.py.  There every reduction already has several contributors -- 16-row chunks over 32 or more token rows and
288 video rows, duplicate ids in an 80-word vocabulary -- so the atomic path these steps replace would differ from run to run.
Every comparison is torch.equal."""
import argparse
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# a small ladder for the small model (three classes), as in tests/test_ragged_train_gpu.py
LADDER = {"query": (8, 16), "his": (8, 16), "cap": (8, 16), "trg": (8, 16), "frames": (8, 16)}
LADDER_STEPS = {"query": 8, "his": 8, "cap": 8, "trg": 8, "frames": 8}


def _args(dropout=0.0):
    from oracle import bist_oracle as O
    cfg = O.Cfg(d_model=64, att_h=4, nb_blocks=2, nb_venc_blocks=2, nb_cenc_blocks=2, dropout=dropout)
    return argparse.Namespace(**{**cfg.__dict__, "d_ff": 4 * cfg.d_model})


def _trainer(dtype, dropout=0.0, **kw):
    """A trainer on a model built after torch.manual_seed(0) and Fn.manual_seed(7): the same weights and dropout seeds every time."""
    import bist_amd.model as M
    from bist_amd import functional as Fn
    from bist_amd.train import Trainer
    args = _args(dropout)
    torch.manual_seed(0)
    Fn.manual_seed(7)
    model = M.make_model(80, 80, args, ft_sizes=[64]).cuda()
    model.train(dropout > 0.0)
    return Trainer(model, args, 80, compute_dtype=dtype, warmup=20, factor=2.0, deterministic=True, **kw)


def _batch(seed, dtype, lo=8, hi=13, T=8, shape_seed=None):
    """B = 4, T = 8 frames of S = 9 regions, C = 64, token lengths 8 .. 12 (drawn from shape_seed, else from seed)."""
    from bist_amd.data.synthetic import synthetic_batch
    rs = np.random.RandomState(seed if shape_seed is None else shape_seed)
    Lq, Lh, Lc, Lt = (int(rs.randint(lo, hi)) for _ in range(4))
    return synthetic_batch(4, T=T, S=9, C=64, Lq=Lq, Lh=Lh, Lc=Lc, Lt=Lt, vocab=80, seed=seed, dtype=dtype)


def _run(tr, batches, grads=False):
    """The steps' loss terms, (the gradient after each step,) and the final master weights and Adam moments."""
    terms, gs = [], []
    for b in batches:
        out = tr.step(b)
        terms.append({k: v.clone() for k, v in out.items()})
        if grads:
            gs.append(tr.flat_grad.clone())
    torch.cuda.synchronize()
    return terms, gs, tr.master.clone(), tr.m.clone(), tr.v.clone()


def _same(a, b, what):
    ta, ga, *sa = a
    tb, gb, *sb = b
    for i, (x, y) in enumerate(zip(ta, tb)):
        assert x.keys() == y.keys()
        for k in x:
            assert torch.equal(x[k], y[k]), "%s: loss term %s of step %d: %r vs %r" % (what, k, i, x[k].item(), y[k].item())
    for i, (x, y) in enumerate(zip(ga, gb)):
        assert torch.equal(x, y), "%s: flat_grad after step %d differs in %d elements" % (what, i, int((x != y).sum()))
    for name, x, y in zip(("master", "m", "v"), sa, sb):
        assert torch.equal(x, y), "%s: %s differs in %d elements" % (what, name, int((x != y).sum()))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "replay"])
def test_two_runs_of_three_steps_with_dropout_are_bit_identical(use_graph, dtype):
    # the same geometry three times: the replayed runs capture once (a new exact shape would be a new capture and new seeds, alike in
    # both runs, but slower)
    runs = []
    for _ in range(2):
        tr = _trainer(dtype, dropout=0.1, use_graph=use_graph)
        batches = [_batch(s, dtype, shape_seed=11) for s in (11, 12, 13)]          # three different batches of one shape
        runs.append(_run(tr, batches))
        del tr
    assert (runs[0][2] != 0).any()
    _same(runs[0], runs[1], "run 1 vs run 2")


def _eager_vs_replay(dtype):
    batches = [_batch(21, dtype)] * 3
    eager = _run(_trainer(dtype), batches, grads=True)
    replay = _run(_trainer(dtype, use_graph=True), batches, grads=True)
    _same(eager, replay, "eager vs replay")
    return eager


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_eager_and_replayed_steps_are_bit_identical_without_dropout(dtype):
    _eager_vs_replay(dtype)


def test_eager_and_replayed_steps_are_bit_identical_on_the_runtime_executor():
    """The same comparison in a child process with BIST_SPLIT_GRAPH=0 (the switch is read at import)."""
    env = dict(os.environ, BIST_SPLIT_GRAPH="0")
    r = subprocess.run([sys.executable, "-s", os.path.abspath(__file__), "--eager-vs-replay"], env=env, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "eager vs replay: identical" in r.stdout


def _classes():
    from bist_amd.data.classes import LengthClasses
    return LengthClasses(LADDER, LADDER_STEPS)


def test_class_step_equals_the_exact_shape_replay_of_the_padded_batch_and_reruns_reproduce():
    dtype = torch.float32
    seeds = [(31, 3, 9, 6), (32, 9, 14, 12), (33, 9, 14, 12)]        # classes "all 8", then "all 16" (frames too) twice: a capture and a hit
    batches = [_batch(s, dtype, lo, hi, T) for s, lo, hi, T in seeds]
    tc = _trainer(dtype, use_graph=True, length_classes=_classes())
    tx = _trainer(dtype, use_graph=True)
    for i, b in enumerate(batches):
        a = tc.step(b)
        padded = copy.copy(tc._static_batch)                       # the class-shaped batch the step just read
        for f in tc._BATCH_FIELDS:
            v = getattr(padded, f, None)
            if v is not None:
                setattr(padded, f, v.clone())
        c = tx.step(padded)
        torch.cuda.synchronize()
        for k in a:
            assert torch.equal(a[k], c[k]), (i, k)
        assert torch.equal(tc.flat_grad, tx.flat_grad), "step %d: %d gradient elements differ" % (i, int((tc.flat_grad != tx.flat_grad).sum()))
        assert torch.equal(tc.master, tx.master), i
    assert tc.graph_stats()["captures"] == 2
    again = _trainer(dtype, use_graph=True, length_classes=_classes())
    for b in batches:
        again.step(b)
    torch.cuda.synchronize()
    assert torch.equal(again.master, tc.master)


def test_evaluate_totals_are_identical_over_two_passes():
    dtype = torch.float32
    tr = _trainer(dtype, use_graph=True, length_classes=_classes())
    batches = [_batch(41, dtype, 3, 9, 6), _batch(42, dtype, 9, 14, 12), _batch(43, dtype, 3, 9, 6)]
    tr.step(batches[0])
    first, second = tr.evaluate(batches), tr.evaluate(batches)
    assert first == second and first["batches"] == 3


def test_the_in_launch_split_k_hint_is_refused():
    from bist_amd import ops
    a, b, c = (torch.zeros(64, 64, device="cuda") for _ in range(3))
    g = ops.gemm_desc(a, b, c, M=64, N=64, K=64, a_rs=64, b_rs=64, ldc=64)
    g.hint = 4
    ops.DETERMINISTIC = True
    try:
        with pytest.raises(RuntimeError, match="split-K"):
            ops.gemm_pair(g, g)
    finally:
        ops.DETERMINISTIC = False


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    assert sys.argv[1:] == ["--eager-vs-replay"]
    from bist_amd import train
    assert not train.SPLIT_GRAPH
    _eager_vs_replay(torch.float32)
    print("eager vs replay: identical")
