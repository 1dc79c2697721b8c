"""The slab reductions inside a Trainer step against the per-workgroup atomics they replace: ops.REDUCE_SLABS "ln" (the default: the
LayerNorm jobs through slabs) and "all" (BIST_REDUCE_SLABS=1: the column sums too) against "0", one layer per stack, d_model = 512
(rows of 1 KiB in bf16, so the LayerNorm parameter gradients ARE deferred to the flush), B = 2, T = 2, no dropout.

All trainers start from the same seed, and no gradient is read back by the pass that produces it, so every reduction of every run is
an fp32 sum, in some order, of the same terms.  EVERY element of the fp32 prefix gradient (acc32) must therefore agree between two
runs within the sum of the two runs' bounds of tests/test_reduce_slab_gpu.py: n * 2^-23 * sum|terms| each, with n and sum|terms|
taken over every job that adds into the element.  The terms come from recorded operands: a deterministic trainer hands every
reduction into acc32 -- bias column sums, LayerNorm gain / offset sums, the stage-2 value bias, the embedding rows -- to one of four
ops functions, which are spied on here; the LayerNorm terms are formed as tests/test_det_reduce_gpu.py forms them."""
import argparse

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23


def _trainer(**kw):
    import bist_amd.model as M
    from bist_amd import functional as Fn
    from bist_amd.train import Trainer
    from oracle import bist_oracle as O
    cfg = O.Cfg(d_model=512, att_h=8, nb_blocks=1, nb_venc_blocks=1, nb_cenc_blocks=1, dropout=0.0)
    args = argparse.Namespace(**{**cfg.__dict__, "d_ff": 4 * cfg.d_model})
    torch.manual_seed(0)
    Fn.manual_seed(7)
    model = M.make_model(80, 80, args, ft_sizes=[64]).cuda()
    model.train(False)
    return Trainer(model, args, 80, compute_dtype=torch.bfloat16, warmup=20, factor=2.0, **kw)


def _batch():
    from bist_amd.data.synthetic import synthetic_batch
    return synthetic_batch(2, T=2, S=9, C=64, Lq=9, Lh=11, Lc=10, Lt=12, vocab=80, seed=5, dtype=torch.bfloat16)


@pytest.fixture(scope="module")
def bounds():
    """Per element of acc32: the number of terms and sum|terms| (fp64) of every reduction that adds into it, recorded from the operands
    of one deterministic step."""
    from bist_amd import ops
    mp = pytest.MonkeyPatch()
    tr = _trainer(deterministic=True)
    n = torch.zeros(tr.n32, device="cuda", dtype=torch.float64)
    mag = torch.zeros(tr.n32, device="cuda", dtype=torch.float64)
    seen = {"col": 0, "ln": 0, "emb": 0, "sb": 0}

    def span(acc, k):
        lo = (acc.data_ptr() - tr.acc32.data_ptr()) // 4
        assert 0 <= lo and lo + k <= tr.n32, "a reduction outside the prefix accumulator"
        return lo

    col_det, ln_det, emb_det, sb_bwd = ops.col_sum_det, ops.lngrad_det, ops.embed_bwd_det, ops.scaled_bias_bwd

    def col_spy(jobs):
        for dz, acc, M, N in jobs:
            lo = span(acc, N)
            n[lo:lo + N] += M
            mag[lo:lo + N] += dz.reshape(-1)[:M * N].view(M, N).double().abs().sum(0)
            seen["col"] += 1
        col_det(jobs)

    def ln_spy(jobs):
        for dy, x, a, da, db, eps in jobs:
            d = x.shape[1]
            xd, gd = x.double(), dy.double()
            term = gd * (xd - xd.mean(1, keepdim=True)) / (xd.std(1, keepdim=True) + eps)
            for acc, t in ((da, term), (db, gd)):
                lo = span(acc, d)
                n[lo:lo + d] += x.shape[0]
                mag[lo:lo + d] += t.abs().sum(0)
            seen["ln"] += 1
        ln_det(jobs)

    def emb_spy(jobs):
        for ids, dy, drop, acc in jobs:
            assert drop is None or drop[0] == 0.0
            V, d = acc.shape
            lo = span(acc, V * d)
            flat = ids.reshape(-1)
            n[lo:lo + V * d].view(V, d).index_add_(0, flat, torch.ones((flat.numel(), d), device="cuda", dtype=torch.float64))
            mag[lo:lo + V * d].view(V, d).index_add_(0, flat, dy.reshape(-1, d).double().abs() * (d ** 0.5))
            seen["emb"] += 1
        emb_det(jobs)

    def sb_spy(dy2, s, bias, ds, acc, h):
        M, d = dy2.shape
        lo = span(acc, d)
        n[lo:lo + d] += M
        mag[lo:lo + d] += (s.double().repeat_interleave(d // h, 1) * dy2.double()).abs().sum(0)
        seen["sb"] += 1
        sb_bwd(dy2, s, bias, ds, acc, h)
    mp.setattr(ops, "col_sum_det", col_spy)
    mp.setattr(ops, "lngrad_det", ln_spy)
    mp.setattr(ops, "embed_bwd_det", emb_spy)
    mp.setattr(ops, "scaled_bias_bwd", sb_spy)
    try:
        tr.step(_batch())
        torch.cuda.synchronize()
    finally:
        mp.undo()
    assert seen["col"] > 0 and seen["ln"] > 0 and seen["emb"] > 0, seen          # (the stage-2 value bias has a reduction of its own only under attention dropout)
    return n, mag, tr.acc32.clone()


def _one_step(monkeypatch, mode):
    """acc32 after one step in the given mode, and how many jobs each flush was handed with / without a registered workspace."""
    from bist_amd import ops
    monkeypatch.setattr(ops, "REDUCE_SLABS", mode)
    tr = _trainer()
    assert (tr._reduce_ws_close is not None) == (mode != "0")
    seen = {"col": 0, "ln": 0}
    col_flush, ln_flush = ops.col_sum_flush, ops.lngrad_flush

    def col_spy():
        seen["col"] += len(ops.COLSUM_QUEUE or [])
        assert (ops.REDUCE_WS is not None) == (mode != "0")
        col_flush()

    def ln_spy():
        seen["ln"] += len(ops.LNGRAD_QUEUE or [])
        ln_flush()
    monkeypatch.setattr(ops, "col_sum_flush", col_spy)
    monkeypatch.setattr(ops, "lngrad_flush", ln_spy)
    tr.step(_batch())
    torch.cuda.synchronize()
    monkeypatch.setattr(ops, "col_sum_flush", col_flush)
    monkeypatch.setattr(ops, "lngrad_flush", ln_flush)
    assert seen["col"] > 10 and seen["ln"] > 3, seen          # both kinds of job were deferred to the flush
    if mode != "0":
        assert (tr._reduce_ws_close[:64].view(torch.int32) == 0).all()
    return tr.acc32.clone()


@pytest.fixture(scope="module")
def atomics_step():
    mp = pytest.MonkeyPatch()
    try:
        return _one_step(mp, "0")
    finally:
        mp.undo()


@pytest.mark.parametrize("mode", ["ln", "all"])
def test_a_step_with_slabs_agrees_with_a_step_with_per_workgroup_atomics_in_every_element(mode, bounds, atomics_step, monkeypatch):
    n, mag, det = bounds
    got, ref = _one_step(monkeypatch, mode), atomics_step
    assert torch.isfinite(got).all() and torch.isfinite(ref).all()
    bound = 2.0 * n * EPS32 * mag                                      # the sum of the two runs' bounds; 0 where nothing adds
    for name, other in (("atomics", ref), ("deterministic", det)):
        err = (got.double() - other.double()).abs()
        ratio = (err / bound.clamp_min(1e-300))[n > 0].max().item()
        print("prefix gradient %s vs %s, %d of %d elements written: max |diff| / bound %.4f" % (mode, name, int((n > 0).sum()), got.numel(), ratio))
        assert (err <= bound).all(), (mode, name, ratio)
