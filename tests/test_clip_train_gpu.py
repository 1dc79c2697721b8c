"""Trainer(max_grad_norm=...): the gradient norm, the clip and the non-finite guard inside the step, at the small
model sizes of tests/test_accumulate_train_gpu.py (d = 64, 2 layers, B = 4, T = 8, S = 9, vocabulary 80).  Every trainer is
deterministic, so that "the same" means torch.equal wherever two runs issue the same arithmetic."""
import argparse
import copy
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LADDER = {"query": (8, 16), "his": (8, 16), "cap": (8, 16), "trg": (8, 16), "frames": (8, 16)}
LADDER_STEPS = {"query": 8, "his": 8, "cap": 8, "trg": 8, "frames": 8}
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
GRAPH = pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "replay"])
TINY = 1e-37                 # below fp32's smallest normal numbers a relative bound says nothing


def _args(dropout=0.0):
    from oracle import bist_oracle as O
    cfg = O.Cfg(d_model=64, att_h=4, nb_blocks=2, nb_venc_blocks=2, nb_cenc_blocks=2, dropout=dropout)
    return argparse.Namespace(**{**cfg.__dict__, "d_ff": 4 * cfg.d_model})


def _trainer(dtype, dropout=0.0, **kw):
    """A deterministic trainer on a model built after torch.manual_seed(0) and Fn.manual_seed(7): the same weights and seeds every time."""
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
    from bist_amd.data.synthetic import synthetic_batch
    rs = np.random.RandomState(seed if shape_seed is None else shape_seed)
    Lq, Lh, Lc, Lt = (int(rs.randint(lo, hi)) for _ in range(4))
    return synthetic_batch(4, T=T, S=9, C=64, Lq=Lq, Lh=Lh, Lc=Lc, Lt=Lt, vocab=80, seed=seed, dtype=dtype)


def _select(batch, idx):
    from bist_amd.data.batch import Batch
    idx = torch.as_tensor(idx, device=batch.query.device)
    return Batch(batch.query[idx], batch.his[idx], batch.fts[idx], batch.cap[idx], batch.trg[idx],
                 batch.trg_y[idx] if batch.trg_y is not None else None)


def _uneven_halves(dtype):
    """The two halves of one B = 4 batch whose clips 2 and 3 lose the second half of their targets."""
    from bist_amd.data.batch import PAD
    from bist_amd.data.synthetic import EOS
    b = _batch(51, dtype, lo=12, hi=13)
    cut = b.trg.shape[1] // 2
    b.trg_y[2:, cut:] = PAD
    b.trg[2:, cut + 1:] = PAD
    b.trg_y[2:, cut - 1] = EOS
    return _select(b, [0, 1]), _select(b, [2, 3])


def _classes():
    from bist_amd.data.classes import LengthClasses
    return LengthClasses(LADDER, LADDER_STEPS)


def _three(dtype):
    return [_batch(s, dtype, shape_seed=11) for s in (11, 12, 13)]              # three different batches of one shape


def _run(tr, batches):
    terms = []
    for b in batches:
        terms.append({k: v.clone() for k, v in tr.step(b).items()})
    torch.cuda.synchronize()
    return terms, tr.master.clone(), tr.m.clone(), tr.v.clone()


def _same(a, b, what):
    ta, *sa = a
    tb, *sb = b
    assert len(ta) == len(tb)
    for i, (x, y) in enumerate(zip(ta, tb)):
        assert x.keys() == y.keys()
        for k in x:
            assert torch.equal(x[k], y[k]), "%s: loss term %s of step %d: %r vs %r" % (what, k, i, x[k].item(), y[k].item())
    for name, x, y in zip(("master", "m", "v"), sa, sb):
        assert torch.equal(x, y), "%s: %s differs in %d elements" % (what, name, int((x != y).sum()))


def _close(x, y, rel, what):
    """Elementwise |x - y| <= rel |y| (+ TINY)."""
    bad = (x.double() - y.double()).abs() > rel * y.double().abs() + TINY
    worst = ((x.double() - y.double()).abs() / (y.double().abs() + TINY)).max().item()
    print("%s: worst relative difference %.3g (bound %.3g)" % (what, worst, rel))
    assert not bad.any(), "%s: %d elements beyond relative %.3g (worst %.3g)" % (what, int(bad.sum()), rel, worst)


@functools.lru_cache(maxsize=None)
def _first_step(dtype):
    """(reference norm of the first batch's gradient from a backward() without optimiser, the plain trainer's m and v after one step)."""
    b = _three(dtype)[0]
    twin = _trainer(dtype)
    twin.backward(b)
    norm = twin.flat_grad.double().norm().item()
    plain = _trainer(dtype)
    plain.step(b)
    torch.cuda.synchronize()
    return norm, plain.m.clone(), plain.v.clone()


# ---- 7. an infinite bound is the plain trainer ---------------------------------------------------------------------------------------
@DTYPES
@GRAPH
def test_an_infinite_bound_is_the_plain_trainer_bit_for_bit(use_graph, dtype):
    batches = _three(dtype)
    plain = _run(_trainer(dtype, dropout=0.1, use_graph=use_graph), batches)     # (with dropout: one trainer at a time, ops.DROP_CTR)
    tr = _trainer(dtype, dropout=0.1, use_graph=use_graph, max_grad_norm=math.inf)
    assert tr.early_adam is False
    clipped = _run(tr, batches)
    assert (plain[1] != 0).any()
    _same(plain, clipped, "plain vs max_grad_norm=inf")
    st = tr.clip_stats()
    assert st["skipped"] == 0 and st["scale"] == 1.0 and st["norm"] > 0 and math.isfinite(st["norm"])


# ---- 8. the norm is the norm -----------------------------------------------------------------------------------------------------------
@DTYPES
@GRAPH
def test_the_norm_is_the_norm_of_the_flat_gradient(use_graph, dtype):
    want = _first_step(dtype)[0]
    tr = _trainer(dtype, use_graph=use_graph, max_grad_norm=math.inf)
    tr.step(_three(dtype)[0])
    got = tr.grad_norm()
    assert got.is_cuda and got.dim() == 0 and got.data_ptr() == tr.hyper.data_ptr() + 24
    print("norm %.9g, reference %.9g" % (got.item(), want))
    assert want > 0 and abs(got.item() - want) <= 1e-6 * want


# ---- 9. clipping scales the moments and reaches the update ---------------------------------------------------------------------------------
@DTYPES
def test_a_bound_of_half_the_norm_halves_m_and_quarters_v(dtype):
    norm, m_plain, v_plain = _first_step(dtype)
    batches = _three(dtype)
    tr = _trainer(dtype, max_grad_norm=0.5 * norm)
    tr.step(batches[0])
    st = tr.clip_stats()
    formula = 0.5 * norm / (norm + 1e-6)
    print("norm %.9g scale %.9g formula %.9g" % (st["norm"], st["scale"], formula))
    assert abs(st["scale"] - formula) <= 1e-6 and st["skipped"] == 0
    _close(tr.m, 0.5 * m_plain, 2e-6, "m against 0.5 m_plain")
    _close(tr.v, 0.25 * v_plain, 2e-6, "v against 0.25 v_plain")
    assert (m_plain != 0).any()
    for b in batches[1:]:
        tr.step(b)
    plain = _trainer(dtype)
    for b in batches:
        plain.step(b)
    torch.cuda.synchronize()
    assert not torch.equal(tr.master, plain.master), "the clip factor never reached the update"
    assert torch.isfinite(tr.master).all()


# ---- 10. eager and replayed clipped steps ------------------------------------------------------------------------------------------------
@DTYPES
def test_eager_and_replayed_clipped_steps_are_bit_identical(dtype):
    bound = 0.5 * _first_step(dtype)[0]
    runs = []
    for use_graph in (False, True):
        tr = _trainer(dtype, use_graph=use_graph, max_grad_norm=bound)
        norms = []
        for b in _three(dtype):
            tr.step(b)
            norms.append(tr.grad_norm().clone())
            assert tr.clip_stats()["scale"] < 1.0, "the bound does not clip this step"
        runs.append((norms, tr.master.clone(), tr.m.clone(), tr.v.clone()))
    for i, (x, y) in enumerate(zip(runs[0][0], runs[1][0])):
        assert torch.equal(x, y), "norm of step %d: %r vs %r" % (i, x.item(), y.item())
    for name, x, y in zip(("master", "m", "v"), runs[0][1:], runs[1][1:]):
        assert torch.equal(x, y), "%s differs in %d elements" % (name, int((x != y).sum()))


# ---- 11. accumulate=True ---------------------------------------------------------------------------------------------------------------
def _spy(tr, use_graph):
    """Record (hyper[5:8], skipped) after every pass of every group."""
    seen = []
    name = "_graph_open" if use_graph else "backward"
    orig = getattr(tr, name)

    def wrapped(*a, **kw):
        out = orig(*a, **kw)
        seen.append((tr.hyper[5:8].clone(), tr.skipped.clone()))
        return out
    setattr(tr, name, wrapped)
    return seen


@DTYPES
def test_a_clipped_group_measures_the_summed_gradient_in_its_last_pass_only(dtype):
    h0, h1 = _uneven_halves(dtype)
    twin = _trainer(dtype, accumulate=True)
    twin.step_group([h0, h1])
    torch.cuda.synchronize()
    one_minus_b1 = float(np.float32(1.0) - np.float32(twin.betas[0]))
    norm_twin = twin.m.double().norm().item() / one_minus_b1
    bound = 0.5 * norm_twin
    runs = []
    for use_graph in (False, True):
        tr = _trainer(dtype, use_graph=use_graph, accumulate=True, max_grad_norm=bound)
        seen = _spy(tr, use_graph)
        tr.step_group([h0, h1])
        st = tr.clip_stats()
        print("group norm %.9g, twin %.9g, scale %.9g" % (st["norm"], norm_twin, st["scale"]))
        assert abs(tr.grad_norm().item() - norm_twin) <= 1e-5 * norm_twin
        assert st["scale"] < 1.0 and st["skipped"] == 0
        _close(tr.m, st["scale"] * twin.m, 4e-6, "m against scale m_twin")
        first = (tr.master.clone(), tr.m.clone(), tr.v.clone(), tr.grad_norm().clone())
        # the first pass of the two-pass group measured nothing: norm and factor still as constructed
        assert len(seen) == 2 and seen[0][0].tolist() == [0.0, 0.0, 0.0] and int(seen[0][1]) == 0
        after_group = (seen[1][0].clone(), seen[1][1].clone())
        assert after_group[0][1].item() == st["norm"] and after_group[0][2].item() == st["scale"]
        tr.step_group([h0, h1, h0])
        torch.cuda.synchronize()
        assert len(seen) == 5
        for k in (2, 3):                                           # first and middle pass of the three-pass group
            assert torch.equal(seen[k][0], after_group[0]) and torch.equal(seen[k][1], after_group[1]), "pass %d changed the statistics" % k
        assert seen[4][0][1].item() != after_group[0][1].item() and int(seen[4][1]) == 0
        runs.append(first + (tr.master.clone(), tr.m.clone(), tr.v.clone(), tr.grad_norm().clone()))
    for i, (x, y) in enumerate(zip(*runs)):
        assert torch.equal(x, y), "eager vs replay: item %d differs" % i


# ---- 12. a non-finite gradient is skipped, not applied -------------------------------------------------------------------------------------
def _state(tr):
    return tr.master.clone(), tr.m.clone(), tr.v.clone(), tr.flat_param.clone()


def _restore(tr, st):
    for dst, src in zip((tr.master, tr.m, tr.v), st):
        dst.copy_(src)
    if tr.flat_param is not tr.master:
        tr.flat_param.copy_(st[3])


def _with_inf(batch):
    bad = copy.copy(batch)
    bad.fts = batch.fts.clone()
    bad.fts.view(-1)[5] = float("inf")
    return bad


@DTYPES
@GRAPH
def test_a_non_finite_gradient_is_skipped_and_the_next_step_trains(use_graph, dtype):
    b0, b1, b2 = _three(dtype)
    tr = _trainer(dtype, use_graph=use_graph, max_grad_norm=math.inf)
    tr.step(b0)
    torch.cuda.synchronize()
    before = _state(tr)
    assert (before[1] != 0).any()
    tr.step(_with_inf(b1))
    st = tr.clip_stats()
    assert st["skipped"] == 1 and st["scale"] == 0.0 and not math.isfinite(st["norm"])
    for name, x, y in zip(("master", "m", "v", "working weights"), _state(tr), before):
        assert torch.equal(x, y), "%s changed in a skipped step" % name
    tr.step(b2)
    st = tr.clip_stats()
    assert st["skipped"] == 1 and st["scale"] == 1.0 and math.isfinite(st["norm"])
    assert not torch.equal(tr.master, before[0])
    # a skipped update consumes its step number: the twin spends step 2 on a finite batch and takes its buffers back
    twin = _trainer(dtype, use_graph=use_graph, max_grad_norm=math.inf)
    twin.step(b0)
    kept = _state(twin)
    twin.step(b1)
    _restore(twin, kept)
    twin.step(b2)
    torch.cuda.synchronize()
    assert twin.clip_stats()["skipped"] == 0 and tr._step == twin._step == 3
    for name, x, y in zip(("master", "m", "v", "working weights"), _state(tr), _state(twin)):
        assert torch.equal(x, y), "%s differs from the twin's in %d elements" % (name, int((x != y).sum()))


@pytest.mark.parametrize("use_graph,dtype", [(False, torch.float32), (True, torch.bfloat16)], ids=["eager-f32", "replay-bf16"])
def test_a_group_whose_second_pass_is_not_finite_is_skipped(use_graph, dtype):
    h0, h1 = _uneven_halves(dtype)
    tr = _trainer(dtype, use_graph=use_graph, accumulate=True, max_grad_norm=math.inf)
    tr.step_group([h0, h1])
    torch.cuda.synchronize()
    before = _state(tr)
    assert (before[1] != 0).any()
    tr.step_group([h0, _with_inf(h1)])
    assert tr.clip_stats()["skipped"] == 1
    for name, x, y in zip(("master", "m", "v", "working weights"), _state(tr), before):
        assert torch.equal(x, y), "%s changed in a skipped group" % name
    tr.step_group([h0, h1])                                       # the first pass overwrites the accumulator: no repair
    st = tr.clip_stats()
    assert st["skipped"] == 1 and math.isfinite(st["norm"]) and st["scale"] == 1.0
    assert not torch.equal(tr.master, before[0])
    assert all(torch.isfinite(x.float()).all() for x in _state(tr))
    assert tr._step == 3 and int(tr.opt_ctr) == 3


# ---- 13. length classes and validation between steps -----------------------------------------------------------------------------------------
def test_clipped_class_steps_equal_the_exact_shape_replays_and_evaluate_changes_nothing():
    dtype = torch.float32
    bound = 1e-3                                                   # far below any gradient norm of this model: every step clips
    batches = [_batch(s, dtype, lo, hi, T) for s, lo, hi, T in ((31, 3, 9, 6), (32, 9, 14, 12))]      # classes "all 8" and "all 16"
    tc = _trainer(dtype, use_graph=True, length_classes=_classes(), max_grad_norm=bound)
    tx = _trainer(dtype, use_graph=True, max_grad_norm=bound)
    for i, b in enumerate(batches):
        tc.step(b)
        padded = copy.copy(tc._static_batch)                       # the class-shaped batch the step just read
        for f in tc._BATCH_FIELDS:
            v = getattr(padded, f, None)
            if v is not None:
                setattr(padded, f, v.clone())
        tx.step(padded)
        torch.cuda.synchronize()
        assert tc.clip_stats()["scale"] < 1.0
        assert torch.equal(tc.m, tx.m), "step %d: %d elements of m differ" % (i, int((tc.m != tx.m).sum()))
        assert torch.equal(tc.master, tx.master) and torch.equal(tc.grad_norm(), tx.grad_norm())
        if i == 0:
            before = _state(tc) + (tc.hyper.clone(), tc.skipped.clone())
            out = tc.evaluate(batches)
            assert out["batches"] == 2
            for x, y in zip(_state(tc) + (tc.hyper.clone(), tc.skipped.clone()), before):
                assert torch.equal(x, y), "evaluate() changed the trainer"
    assert tc.graph_stats()["captures"] == 2
