"""Trainer(accumulate=True): one optimiser step over several batches, at the small model sizes of
tests/test_deterministic_train_gpu.py (d = 64, 2 layers, B = 4, T = 8, S = 9, vocabulary 80).  Every trainer is deterministic, so that
"the same" means torch.equal wherever two runs issue the same arithmetic."""
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

# a small ladder for the small model, as in tests/test_deterministic_train_gpu.py
LADDER = {"query": (8, 16), "his": (8, 16), "cap": (8, 16), "trg": (8, 16), "frames": (8, 16)}
LADDER_STEPS = {"query": 8, "his": 8, "cap": 8, "trg": 8, "frames": 8}


def _args(dropout=0.0):
    from oracle import bist_oracle as O
    cfg = O.Cfg(d_model=64, att_h=4, nb_blocks=2, nb_venc_blocks=2, nb_cenc_blocks=2, dropout=dropout)
    return argparse.Namespace(**{**cfg.__dict__, "d_ff": 4 * cfg.d_model})


def _trainer(dtype, dropout=0.0, deterministic=True, **kw):
    """A trainer on a model built after torch.manual_seed(0) and Fn.manual_seed(7): the same weights and dropout seeds every time."""
    import bist_amd.model as M
    from bist_amd import functional as Fn
    from bist_amd.train import Trainer
    args = _args(dropout)
    torch.manual_seed(0)
    Fn.manual_seed(7)
    model = M.make_model(80, 80, args, ft_sizes=[64]).cuda()
    model.train(dropout > 0.0)
    return Trainer(model, args, 80, compute_dtype=dtype, warmup=20, factor=2.0, deterministic=deterministic, **kw)


def _batch(seed, dtype, lo=8, hi=13, T=8, shape_seed=None):
    """B = 4, T = 8 frames of S = 9 regions, C = 64, token lengths 8 .. 12 (drawn from shape_seed, else from seed)."""
    from bist_amd.data.synthetic import synthetic_batch
    rs = np.random.RandomState(seed if shape_seed is None else shape_seed)
    Lq, Lh, Lc, Lt = (int(rs.randint(lo, hi)) for _ in range(4))
    return synthetic_batch(4, T=T, S=9, C=64, Lq=Lq, Lh=Lh, Lc=Lc, Lt=Lt, vocab=80, seed=seed, dtype=dtype)


def _select(batch, idx):
    from bist_amd.data.batch import Batch
    idx = torch.as_tensor(idx, device=batch.query.device)
    return Batch(batch.query[idx], batch.his[idx], batch.fts[idx], batch.cap[idx], batch.trg[idx],
                 batch.trg_y[idx] if batch.trg_y is not None else None)


def _classes():
    from bist_amd.data.classes import LengthClasses
    return LengthClasses(LADDER, LADDER_STEPS)


def _run(tr, items, group):
    """The loss terms of every step (step(item)) or group (step_group(item)) and the final master weights and Adam moments."""
    terms = []
    for it in items:
        out = tr.step_group(it) if group else tr.step(it)
        terms.append({k: v.clone() for k, v in out.items()})
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


# ---- 1. a group of one is a plain step -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "replay"])
def test_a_group_of_one_is_a_plain_step(use_graph, dtype):
    batches = [_batch(s, dtype, shape_seed=11) for s in (11, 12, 13)]              # three different batches of one shape
    plain = _run(_trainer(dtype, dropout=0.1, use_graph=use_graph), batches, group=False)
    ta = _trainer(dtype, dropout=0.1, use_graph=use_graph, accumulate=True)
    acc = _run(ta, batches, group=False)                                           # step() of such a trainer is step_group([batch])
    assert (plain[1] != 0).any() and ta._step == 3 and int(ta.drop_ctr) == 3
    _same(plain, acc, "plain vs accumulate=True")


# ---- 2. a group equals the big batch -----------------------------------------------------------------------------------------
def _uneven_batch(dtype):
    """One B = 4 batch whose clips 2 and 3 lose the second half of their targets: (full, half0, half1)."""
    from bist_amd.data.batch import PAD
    from bist_amd.data.synthetic import EOS
    b = _batch(51, dtype, lo=12, hi=13)
    Lt = b.trg.shape[1]
    cut = Lt // 2
    b.trg_y[2:, cut:] = PAD
    b.trg[2:, cut + 1:] = PAD
    b.trg_y[2:, cut - 1] = EOS
    return _select(b, [0, 1, 2, 3]), _select(b, [0, 1]), _select(b, [2, 3])


def _group_vs_full(dtype):
    full, h0, h1 = _uneven_batch(dtype)
    n0, n1 = int(h0.ntokens), int(h1.ntokens)
    assert abs(n0 - n1) >= 0.25 * max(n0, n1), (n0, n1)
    assert n0 + n1 == int(full.ntokens) and int(h0.qntokens) + int(h1.qntokens) == int(full.qntokens)
    # (two trainers alive at once: Trainer.__init__ rebinds the module-wide ops.DROP_CTR to the newest trainer's counter, so the older
    # one would read the other's dropout counter -- harmless only because dropout is off here; with dropout, build and step one at a time)
    tg, tf = _trainer(dtype, accumulate=True), _trainer(dtype)
    a = tg.step_group([h0, h1])
    c = tf.step(full)
    torch.cuda.synchronize()
    assert tg._step == 1 and tf._step == 1
    assert a.keys() == c.keys()
    for k in a:
        x, y = a[k].item(), c[k].item()
        print("%s term %s: group %.9g full %.9g rel %.3g" % (dtype, k, x, y, abs(x - y) / abs(y)))
    return tg, tf, a, c


def test_a_group_of_two_uneven_halves_is_the_step_on_the_whole_batch_f32():
    """Fails when each pass is normalised by its own token counts (the halves' counts differ by half)."""
    tg, tf, a, c = _group_vs_full(torch.float32)
    worst = 0.0
    for lo, hi in tf.pieces:
        mg, mf = tg.m[lo:hi], tf.m[lo:hi]
        scale = mf.abs().max().item()
        err = (mg - mf).abs().max().item()
        worst = max(worst, err / scale)
        print("piece [%d, %d): max |m_group - m_full| %.3g, max |m_full| %.3g" % (lo, hi, err, scale))
        assert scale > 0 and err <= 2e-4 * scale, (lo, hi, err, scale)
    for k in a:
        assert abs(a[k].item() - c[k].item()) <= 1e-5 * abs(c[k].item()), (k, a[k].item(), c[k].item())


def test_a_group_of_two_uneven_halves_is_the_step_on_the_whole_batch_bf16():
    tg, tf, a, c = _group_vs_full(torch.bfloat16)
    scale = tf.m.abs().max().item()
    err = (tg.m - tf.m).abs().max().item()
    rel = ((tg.m - tf.m).norm() / tf.m.norm()).item()
    print("bf16: max error %.3g of %.3g, relative norm %.3g" % (err, scale, rel))
    assert scale > 0 and torch.isfinite(tg.m).all()
    assert err <= 4e-2 * scale, (err, scale)
    assert rel <= 2e-2, rel


# ---- 3. the two counters ------------------------------------------------------------------------------------------------------
def test_the_dropout_counter_counts_passes_and_the_optimiser_counter_updates():
    dtype = torch.float32
    tr = _trainer(dtype, dropout=0.1, accumulate=True)
    b = _batch(61, dtype)
    tr.step_group([b, b, b])
    assert int(tr.drop_ctr) == 3 and tr._step == 1 and int(tr.opt_ctr) == 1
    assert np.float32(tr.hyper[0].item()) == np.float32(tr.rate(1))
    tr.step_group([b, b])
    assert int(tr.drop_ctr) == 5 and tr._step == 2 and int(tr.opt_ctr) == 2
    assert np.float32(tr.hyper[0].item()) == np.float32(tr.rate(2))
    # (the bias correction of update 2, from beta1 as the launch receives it: a C float, raised in double)
    assert np.float32(tr.hyper[1].item()) == np.float32(1 - float(np.float32(tr.betas[0])) ** 2)


# ---- 4. reproducible and replay-exact -----------------------------------------------------------------------------------------
def _groups(dtype):
    return [[_batch(s, dtype, shape_seed=71) for s in seeds] for seeds in ((71, 72, 73), (74, 75, 76))]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_two_runs_of_two_replayed_groups_with_dropout_are_bit_identical(dtype):
    runs = []
    for _ in range(2):
        tr = _trainer(dtype, dropout=0.1, use_graph=True, accumulate=True)
        runs.append(_run(tr, _groups(dtype), group=True))
        assert tr._step == 2 and int(tr.drop_ctr) == 6
        del tr
    assert (runs[0][1] != 0).any()
    _same(runs[0], runs[1], "run 1 vs run 2")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_eager_and_replayed_groups_are_bit_identical_without_dropout(dtype):
    eager = _run(_trainer(dtype, accumulate=True), _groups(dtype), group=True)
    replay = _run(_trainer(dtype, use_graph=True, accumulate=True), _groups(dtype), group=True)
    _same(eager, replay, "eager vs replay")


# ---- 5. length classes --------------------------------------------------------------------------------------------------------
def test_a_group_over_two_length_classes_equals_the_exact_shape_groups_of_the_padded_batches():
    dtype = torch.float32
    # classes "all 8" and "all 16" (frames too) in one group, then the same two classes again: two captures, then two hits
    groups = [[_batch(s, dtype, lo, hi, T) for s, lo, hi, T in g] for g in (((31, 3, 9, 6), (32, 9, 14, 12)), ((33, 3, 9, 6), (34, 9, 14, 12)))]
    # (both trainers alive and stepped in turn: dropout must stay off here, see _group_vs_full on ops.DROP_CTR)
    tc = _trainer(dtype, use_graph=True, length_classes=_classes(), accumulate=True)
    tx = _trainer(dtype, use_graph=True, accumulate=True)
    for i, grp in enumerate(groups):
        a = tc.step_group(grp)
        padded = []
        for b in grp:                                              # each class once per group: its static batch still holds this pass
            static = tc._entries[tc.length_classes.key(b)].batch
            pb = copy.copy(static)
            for f in tc._BATCH_FIELDS:
                v = getattr(static, f, None)
                if v is not None:
                    setattr(pb, f, v.clone())
            assert int(pb.ntokens) == sum(int(x.ntokens) for x in grp)          # the pass was staged with the group's totals ...
            pb.ntokens, pb.qntokens = b.ntokens.clone(), b.qntokens.clone()     # ... the twin sums the batches' own counts itself
            padded.append(pb)
        c = tx.step_group(padded)
        torch.cuda.synchronize()
        for k in a:
            assert torch.equal(a[k], c[k]), (i, k)
        assert torch.equal(tc.master, tx.master), "group %d: %d weights differ" % (i, int((tc.master != tx.master).sum()))
        st = tc.graph_stats()
        assert st["captures"] == 2 and st["hits"] == 2 * i and st["evictions"] == 0, st
    assert tc._step == 2 and int(tc.drop_ctr) == 4


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_in_process(monkeypatch):
    import torch.distributed as dist
    dtype = torch.float32
    with pytest.raises(ValueError, match="deferred_adam"):
        _trainer(dtype, use_graph=True, accumulate=True, deferred_adam=True)
    tr = _trainer(dtype, accumulate=True)
    with pytest.raises(ValueError, match="empty"):
        tr.step_group([])
    assert tr._step == 0
    plain = _trainer(dtype)
    with pytest.raises(ValueError, match="accumulate=True"):
        plain.step_group([_batch(81, dtype)])
    # several ranks, as Trainer.__init__ sees them (two processes and a collective backend are not needed to be refused)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(ValueError, match="several ranks"):
        _trainer(dtype, accumulate=True)


@pytest.mark.parametrize("var,value,word", [("BIST_FORCE_EXCHANGE", "1", "BIST_FORCE_EXCHANGE"), ("BIST_ADAM_IN_STEP", "0", "BIST_ADAM_IN_STEP"),
                                            ("BIST_ADAM_CLEARS", "1", "BIST_ADAM_CLEARS")])
def test_refusals_of_environment_switches(var, value, word):
    """Each switch in a child process of its own (BIST_ADAM_CLEARS is read at import)."""
    env = dict(os.environ, **{var: value})
    r = subprocess.run([sys.executable, "-s", os.path.abspath(__file__), "--refused", word], env=env, capture_output=True, text=True,
                       cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "refused: " + word in r.stdout


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    assert len(sys.argv) == 3 and sys.argv[1] == "--refused"
    try:
        _trainer(torch.float32, accumulate=True)
    except ValueError as e:
        assert sys.argv[2] in str(e), str(e)
        print("refused: " + sys.argv[2])
    else:
        raise SystemExit("Trainer(accumulate=True) accepted %s" % sys.argv[2])
    _trainer(torch.float32)                 # the default trainer takes the switch as before
