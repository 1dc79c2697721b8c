"""Validation on ragged batches (Trainer.eval_step / Trainer.evaluate): one forward-only captured step per length class in a bounded
store of its own, the epoch's totals accumulated on the device (bist_eval_accumulate), graphs that stay valid across weight updates.

The yardstick is always code that does not go through the new entry points: a FRESH model loaded from the trainer's model's
``state_dict()`` (so none of the derived buffers the captured graphs read is touched), in ``eval()`` under ``torch.no_grad()``,
``model.forward`` on the same UNPADDED batch and ``SimpleLossCompute.terms`` over that model's heads.  Tolerances: loss terms against
that eager evaluation 1e-5 relative in fp32 and 2e-2 in bf16 (tests/test_ragged_train_gpu.py); against the CPU oracle 1e-3 in fp32.
Model size and helpers follow tests/test_ragged_train_gpu.py, with dropout 0.1 and the trainer's model left in train() mode, so that
eval mode has something to switch off."""
import argparse
import copy
import os
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# a small ladder for the small model: three classes below
SMALL = {"query": (8, 16), "his": (8, 16), "cap": (8, 16), "trg": (8, 16), "frames": (8, 16)}
STEPS = {"query": 8, "his": 8, "cap": 8, "trg": 8, "frames": 8}
SEQ12 = [("A", 11), ("B", 12), ("A", 13), ("B", 14), ("C", 15), ("A", 16), ("C", 17), ("B", 18), ("C", 19), ("A", 20), ("B", 21), ("C", 22)]


def _tol(dtype):
    return 1e-5 if dtype == torch.float32 else 2e-2


def _args():
    from oracle import bist_oracle as O
    cfg = O.Cfg(d_model=64, att_h=4, nb_blocks=2, nb_venc_blocks=2, nb_cenc_blocks=2)
    return argparse.Namespace(**{**cfg.__dict__, "d_ff": 4 * cfg.d_model, "dropout": 0.1})


def _model(args, vocab=80, feat=64):
    import bist_amd.model as M
    torch.manual_seed(0)
    return M.make_model(vocab, vocab, args, ft_sizes=[feat]).cuda().train()


def _classes():
    from bist_amd.data.classes import LengthClasses
    return LengthClasses(SMALL, STEPS)


def _batch(cls: str, seed: int, dtype=torch.float32, B: int = 4):
    """A ragged batch of class 'A' (everything <= 8), 'B' (query 9..16) or 'C' (frames 9..16, history 9..16)."""
    from bist_amd.data.synthetic import synthetic_batch
    rs = np.random.RandomState(seed)
    Lq, Lh, Lc, Lt, T = (int(rs.randint(3, 9)) for _ in range(5))
    if cls == "B":
        Lq = int(rs.randint(9, 17))
    if cls == "C":
        T, Lh = int(rs.randint(9, 17)), int(rs.randint(9, 17))
    return synthetic_batch(B, T=T, S=9, C=64, Lq=Lq, Lh=Lh, Lc=Lc, Lt=Lt, vocab=80, seed=seed, dtype=dtype)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _trainer(dtype=torch.float32, model=None, seed=1234, **kw):
    """A class-mode graph trainer on a dropout-0.1 model in train() mode (Fn.manual_seed first: trainers that are compared draw the
    same training-mode masks)."""
    from bist_amd import functional as Fn
    from bist_amd.train import Trainer
    args = _args()
    Fn.manual_seed(seed)
    m = _model(args) if model is None else model
    kw.setdefault("warmup", 20)
    kw.setdefault("factor", 0.0)
    t = Trainer(m, args, 80, compute_dtype=dtype, use_graph=True, length_classes=_classes(), **kw)
    assert m.training
    return t, args


def _eager_copy(model, args, dtype, vocab=80, feat=64):
    """A fresh model with the present weights of `model` (through state_dict(): reads parameters only, runs no forward pass), in the
    compute dtype, eval mode."""
    import bist_amd.model as M
    fresh = M.make_model(vocab, vocab, args, ft_sizes=[feat])
    sd = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
    missing, unexpected = fresh.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith(".pe") for k in missing), (missing, unexpected)
    return fresh.cuda().to(dtype).eval()


def _eager_terms(ref_model, trainer, args, b):
    """The parent commit's validation arithmetic for one batch: eval(), no_grad, model.forward, SimpleLossCompute.terms -> floats."""
    from bist_amd.model.optimize import SimpleLossCompute
    lc = SimpleLossCompute(ref_model.generator, ref_model.ae_generator, trainer.criterion, opt=None, args=args)
    assert not ref_model.training
    with torch.no_grad():
        ft = ref_model.forward(b)
        terms, _ = lc.terms(ft, b)
    torch.cuda.synchronize()
    return {k: v.double().item() for k, v in terms.items()}


def _floats(terms):
    torch.cuda.synchronize()
    return {k: v.double().item() for k, v in terms.items()}


def _close(got, want, tol, what):
    assert set(got) >= set(want), (what, sorted(got), sorted(want))
    for k, w in want.items():
        print("%s %s: got %.9g want %.9g rel %.3e (tol %.1e)" % (what, k, got[k], w, abs(got[k] - w) / max(abs(w), 1e-30), tol))
    for k, w in want.items():
        assert abs(got[k] - w) <= tol * abs(w), (what, k, got[k], w)


def _epoch(per_batch):
    """run_epoch's accumulation (train.py:32-37, 49-51) over [(terms as per-token floats, ntokens, qntokens)] in double."""
    tok = sum(n for _, n, _ in per_batch)
    qtok = sum(q for _, _, q in per_batch)
    out = {}
    for k in per_batch[0][0]:
        out[k] = sum(t[k] * (n if k == "out" else q) for t, n, q in per_batch) / (tok if k == "out" else qtok)
    return out, tok, qtok


def _eager_epoch(ref_model, trainer, args, batches):
    return _epoch([(_eager_terms(ref_model, trainer, args, b), int(b.ntokens.item()), int(b.qntokens.item())) for b in batches])


LOSS_KEYS = ("out", "cap_ae", "temporal_ae", "spatial_ae")


# ---- 1: the class step is the eager evaluation -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_class_eval_step_matches_eager_evaluation(dtype):
    t, args = _trainer(dtype)
    ref = _eager_copy(t.model, args, dtype)
    lc = _classes()
    assert len({lc.key(_batch(c, s)) for c, s in SEQ12}) == 3
    for cls, seed in SEQ12:
        b = _batch(cls, seed, dtype)
        got = _floats(t.eval_step(b))
        want = _eager_terms(ref, t, args, b)
        assert set(got) == set(want) == set(LOSS_KEYS)
        _close(got, want, _tol(dtype), "%s%d" % (cls, seed))
    st = t.eval_graph_stats()
    assert st["captures"] == 3 and st["hits"] == 9 and st["evictions"] == 0 and st["entries"] == 3 and st["bytes"] > 0, st
    assert st["max_eval_graphs"] == t.max_eval_graphs
    g = t.graph_stats()
    assert g["captures"] == 0 and g["hits"] == 0 and g["evictions"] == 0 and g["entries"] == 0 and g["bytes"] == 0, g
    assert t.model.training and t._step == 0 and int(t.drop_ctr.item()) == 0


# ---- 2: against the CPU oracle -----------------------------------------------------------------------------------------------------
def test_evaluate_matches_the_oracle_epoch():
    from oracle import bist_oracle as O
    import bist_amd.model as M
    from bist_amd import functional as Fn
    from bist_amd.data.batch import Batch
    from bist_amd.train import Trainer
    V, C = 80, 64
    args = _args()
    cfg = O.Cfg(d_model=64, att_h=4, nb_blocks=2, nb_venc_blocks=2, nb_cenc_blocks=2)
    sd = O.det_state(cfg, V, C)
    model = M.make_model(V, V, args, ft_sizes=[C])
    model.load_state_dict(sd, strict=False)
    model = model.cuda().train()
    Fn.manual_seed(1234)
    t = Trainer(model, args, V, compute_dtype=torch.float32, warmup=20, factor=0.0, use_graph=True, length_classes=_classes())
    geoms = [dict(T=6, Lq=7, Lh=8, Lc=6, Lt=6), dict(T=7, Lq=12, Lh=8, Lc=5, Lt=7), dict(T=12, Lq=6, Lh=14, Lc=8, Lt=8)]
    obs = [O.det_batch(3, g["T"], 9, C, g["Lq"], g["Lh"], g["Lc"], g["Lt"], V, seed=40 + i) for i, g in enumerate(geoms)]
    batches = [Batch(ob.query.cuda(), ob.his.cuda(), ob.fts.cuda(), ob.cap.cuda(), ob.trg.cuda(), ob.trg_y.cuda()) for ob in obs]
    assert len({t.length_classes.key(b) for b in batches}) >= 2
    per = []
    with torch.no_grad():
        for ob in obs:
            losses = O.loss_compute(sd, cfg, O.mtn_forward(sd, cfg, ob), ob, V)
            per.append(({k: float(losses[k]) for k in LOSS_KEYS if k in losses}, int(ob.ntokens), int(ob.qntokens)))
    want, tok, qtok = _epoch(per)
    got = t.evaluate(batches)
    _close(got, want, 1e-3, "oracle")
    assert got["tokens"] == tok and got["qtokens"] == qtok and got["batches"] == 3


# ---- 3: weights move, graphs stay --------------------------------------------------------------------------------------------------
def _derived_operands(model):
    """(fragment-ordered matrices, packed value projections) the reasoning layers hold, each compared BIT FOR BIT with a fresh pack of
    the present parameters into new buffers (the held buffers are only read)."""
    from bist_amd import functional as Fn, ops
    n_frag = n_vpack = 0
    for l, vl in enumerate(model.mutlimodal_decoder.v_layers):
        for ai, hit in (vl.__dict__.get("_frag_cache") or {}).items():
            for j, held in ((2, hit[1]), (3, hit[2])):
                w = vl.attn[ai].linears[j].weight.detach()
                assert torch.equal(held, ops.pack_frag_rows(w)), "layer %d attention %d: fragment-ordered linears[%d] is stale" % (l, ai, j)
                n_frag += 1
        hit = vl.__dict__.get("_vpack")
        if hit is not None:
            a1, a4 = vl.attn[1].linears[2], vl.attn[4].linears[2]
            with torch.no_grad():
                assert torch.equal(hit[1], Fn.pack_rows(a1.weight, a4.weight)), "layer %d: packed value weights are stale" % l
                assert torch.equal(hit[2], Fn.pack_rows(a1.bias, a4.bias)), "layer %d: packed value biases are stale" % l
            n_vpack += 1
    torch.cuda.synchronize()
    return n_frag, n_vpack


def _weights_move_graphs_stay(t, args, dtype, eval_batches, step_batches, tol, moved_by, copy_kw, want_derived):
    from bist_amd import ops
    ref0 = _eager_copy(t.model, args, dtype, **copy_kw)
    e0, tok, qtok = _eager_epoch(ref0, t, args, eval_batches)
    del ref0
    repacked, orig = [], ops.refresh_inference_operands

    def recording(root):
        repacked.append(orig(root))
        return repacked[-1]
    ops.refresh_inference_operands = recording
    try:
        r0 = t.evaluate(eval_batches)
        _close(r0, e0, tol, "first pass")
        caps = t.eval_graph_stats()["captures"]
        assert caps >= 2
        for b in step_batches:
            t.step(b)
        r1 = t.evaluate(eval_batches)
    finally:
        ops.refresh_inference_operands = orig
    st = t.eval_graph_stats()
    assert st["captures"] == caps and st["evictions"] == 0, st           # the second pass replays the first pass's graphs
    # the operands those graphs read, directly: every buffer holds the present weights, and the one refresh after the steps (the last
    # entry: earlier ones ran before a capture's warm-up passes had built anything, or found nothing changed) re-packed all of them
    held = _derived_operands(t.model)
    print("derived operands held (fragment-ordered matrices, packed value projections) %s, re-packed per refresh %s" % (held, repacked))
    assert held == want_derived and repacked[-1] == want_derived[0] and len(repacked) <= 2, (held, repacked)
    # only NOW the yardstick: an eager forward on the trainer's own model would re-pack the derived operands the graphs read
    ref1 = _eager_copy(t.model, args, dtype, **copy_kw)
    e1, _, _ = _eager_epoch(ref1, t, args, eval_batches)
    print("out: eager before %.9g after %.9g, evaluate before %.9g after %.9g" % (e0["out"], e1["out"], r0["out"], r1["out"]))
    assert abs(e1["out"] - e0["out"]) > moved_by * tol * abs(e0["out"]), ("the steps did not move the loss: the test is void", e0, e1)
    _close(r1, e1, tol, "second pass")
    assert r1["tokens"] == tok and r1["qtokens"] == qtok and r1["batches"] == len(eval_batches)


def test_graphs_survive_weight_updates():
    t, args = _trainer(torch.float32, factor=2.0, warmup=20)
    ev = [_batch(c, 100 + s) for c, s in SEQ12[:6]]
    st = [_batch(c, s) for c, s in SEQ12[:6]]
    # at this width no fragment-ordered weights exist; each of the two reasoning layers holds one packed value projection
    _weights_move_graphs_stay(t, args, torch.float32, ev, st, _tol(torch.float32), 100, {}, (0, 2))
    assert t.graph_stats()["captures"] == 3 and t._step == 6


def test_eager_fallback_without_graphs():
    """Without use_graph / length classes eval_step and evaluate run the same computation as eager launches (the accumulation launch
    included) and capture nothing."""
    from bist_amd import functional as Fn
    from bist_amd.train import Trainer
    args = _args()
    Fn.manual_seed(1234)
    t = Trainer(_model(args), args, 80, compute_dtype=torch.float32, warmup=20, factor=0.0)
    ref = _eager_copy(t.model, args, torch.float32)
    batches = [_batch(c, s) for c, s in SEQ12[:3]]
    for b in batches:
        _close(_floats(t.eval_step(b)), _eager_terms(ref, t, args, b), _tol(torch.float32), "eager step")
    want, tok, qtok = _eager_epoch(ref, t, args, batches)
    got = t.evaluate(batches)
    _close(got, want, _tol(torch.float32), "eager epoch")
    assert (got["tokens"], got["qtokens"], got["batches"]) == (tok, qtok, 3)
    st = t.eval_graph_stats()
    assert st["captures"] == 0 and st["entries"] == 0 and st["hits"] == 0, st
    assert t.model.training and t._step == 0 and int(t.drop_ctr.item()) == 0


# ---- 4: evaluation leaves training alone -------------------------------------------------------------------------------------------
def test_evaluation_leaves_training_alone():
    seq = SEQ12[:6]
    ev = [_batch(c, 200 + s) for c, s in (("A", 1), ("B", 2), ("C", 3), ("A", 4))]

    def run(evaluate_after=None):
        t, _ = _trainer(torch.float32, factor=2.0, warmup=20)
        for i, (cls, seed) in enumerate(seq):
            if evaluate_after == i:
                before = (t._step, int(t.drop_ctr.item()), t.model.training, t.flat_grad.clone(), t.m.clone(), t.v.clone(), t.master.clone())
                res = t.evaluate(ev)
                assert res["batches"] == 4
                torch.cuda.synchronize()
                assert (t._step, int(t.drop_ctr.item()), t.model.training) == before[:3] and t.model.training
                for a, b_ in zip((t.flat_grad, t.m, t.v, t.master), before[3:]):
                    assert torch.equal(a, b_)
            t.step(_batch(cls, seed))
        torch.cuda.synchronize()
        return t
    x = run()
    xm, xs = x.master.clone(), x.graph_stats()
    del x
    y = run(evaluate_after=3)
    ym, ys = y.master.clone(), y.graph_stats()
    assert y.eval_graph_stats()["captures"] == 3
    del y
    z = run()
    zm = z.master.clone()
    spread, apart = _rel(zm, xm), _rel(ym, xm)
    print("masters: with evaluation vs without %.3e, run-to-run %.3e" % (apart, spread))
    assert apart <= max(10 * spread, 1e-6), (apart, spread)
    print("graph_stats: without evaluation %s, with %s" % (xs, ys))
    assert ys == xs, (ys, xs)


# ---- 5: dropout is off and the pass is repeatable ----------------------------------------------------------------------------------
def test_dropout_is_off_and_the_step_repeats():
    t, args = _trainer(torch.float32)
    ref = _eager_copy(t.model, args, torch.float32)
    b = _batch("C", 301)
    a1 = _floats(t.eval_step(b))
    a2 = _floats(t.eval_step(b))
    want = _eager_terms(ref, t, args, b)
    _close(a2, a1, 1e-6, "repeat")
    _close(a1, want, _tol(torch.float32), "eager")
    assert t.model.training
    _, terms = t.forward_loss(b)                      # the trainer's model as it was left: train() mode, dropout on
    tr = _floats({k: v.detach() for k, v in terms.items()})
    for k, w in a1.items():
        print("%s: dropout on %.9g, off %.9g" % (k, tr[k], w))
        assert abs(tr[k] - w) > 10 * _tol(torch.float32) * abs(w), (k, tr[k], w)


# ---- 6: bounded store --------------------------------------------------------------------------------------------------------------
def test_eval_store_is_bounded_and_evictions_keep_the_results():
    t, args = _trainer(torch.float32, max_eval_graphs=2)
    ref = _eager_copy(t.model, args, torch.float32)
    for cls, seed in SEQ12[:8]:
        b = _batch(cls, seed)
        _close(_floats(t.eval_step(b)), _eager_terms(ref, t, args, b), _tol(torch.float32), "%s%d" % (cls, seed))
    st = t.eval_graph_stats()
    # A B A B C A C B with room for two: C evicts A, A evicts B, B evicts A
    assert st["entries"] == 2 and st["captures"] == 5 and st["hits"] == 3 and st["evictions"] == 3 and st["max_eval_graphs"] == 2, st


# ---- 7: epoch totals on the device -------------------------------------------------------------------------------------------------
def test_evaluate_accumulates_the_epoch_on_the_device():
    t, args = _trainer(torch.float32)
    batches = [_batch(c, s) for c, s in SEQ12]
    per = [(_floats(t.eval_step(b)), int(b.ntokens.item()), int(b.qntokens.item())) for b in batches]
    want, tok, qtok = _epoch(per)
    got = t.evaluate(batches)
    _close(got, want, 1e-6, "epoch")
    assert got["tokens"] == tok and got["qtokens"] == qtok and got["batches"] == 12
    assert set(got) == set(LOSS_KEYS) | {"tokens", "qtokens", "batches"}
    again = t.evaluate(batches)                        # starts from zero totals
    _close(again, {k: got[k] for k in LOSS_KEYS}, 1e-6, "second evaluate")
    assert again["tokens"] == tok and again["qtokens"] == qtok and again["batches"] == 12
    assert t.eval_graph_stats()["captures"] == 3


# ---- 8: fed batches ----------------------------------------------------------------------------------------------------------------
def test_evaluate_takes_a_device_feeder():
    from bist_amd.data.feeder import DeviceFeeder, HostBatch
    t, args = _trainer(torch.float32)
    batches = [_batch(c, s) for c, s in SEQ12[:6]]
    want = t.evaluate(batches)
    host = [HostBatch(b.query.cpu(), b.his.cpu(), b.fts.cpu(), b.cap.cpu(), b.trg.cpu(), b.trg_y.cpu()) for b in batches]
    feeder = DeviceFeeder(host, feature_dtype=torch.float32, length_classes=_classes())
    seen = []

    def watched():
        for b in feeder:
            seen.append(b)
            yield b
    got = t.evaluate(watched())
    _close(got, {k: want[k] for k in LOSS_KEYS}, 1e-6, "fed")
    assert (got["tokens"], got["qtokens"], got["batches"]) == (want["tokens"], want["qtokens"], 6)
    assert len(seen) == 6 and all("query_mask" not in b.__dict__ and "temporal_mask" not in b.__dict__ for b in seen), "masks were read"
    assert t.eval_graph_stats()["captures"] == 3


# ---- 9: two ranks ------------------------------------------------------------------------------------------------------------------
RANK_SEQ = [("A", 401), ("C", 402), ("B", 403), ("B", 404), ("A", 405), ("C", 406)]


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    t, _ = _trainer(torch.float32)
    assert t.world == world
    res = t.evaluate([_batch(c, s) for c, s in RANK_SEQ[3 * rank: 3 * rank + 3]])
    torch.cuda.synchronize()
    q.put((rank, res, t.eval_graph_stats()))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_return_the_global_averages():
    import torch.multiprocessing as mp
    t, _ = _trainer(torch.float32)
    want = t.evaluate([_batch(c, s) for c, s in RANK_SEQ])
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = {}
    for _ in range(world):
        r, res, stats = q.get(timeout=300)
        got[r] = (res, stats)
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    assert got[0][0] == got[1][0], (got[0][0], got[1][0])
    for r in range(world):
        res, stats = got[r]
        _close(res, {k: want[k] for k in LOSS_KEYS}, 1e-5, "rank %d" % r)
        assert (res["tokens"], res["qtokens"], res["batches"]) == (want["tokens"], want["qtokens"], 6)
        assert stats["captures"] == 3 and stats["hits"] == 0, stats


# ---- the production kernels' size --------------------------------------------------------------------------------------------------
PV, PC = 3000, 2048


def _prod_args():
    from oracle import bist_oracle as O
    cfg = O.Cfg(d_model=512, att_h=8, nb_blocks=2, nb_venc_blocks=2, nb_cenc_blocks=2)
    return argparse.Namespace(**{**cfg.__dict__, "d_ff": 4 * cfg.d_model, "dropout": 0.1})


def _prod_batch(T, seed, B=4):
    from bist_amd.data.synthetic import synthetic_batch
    rs = np.random.RandomState(seed)
    return synthetic_batch(B, T=T, S=49, C=PC, Lq=int(rs.randint(12, 21)), Lh=int(rs.randint(30, 61)), Lc=int(rs.randint(12, 26)),
                           Lt=int(rs.randint(10, 21)), vocab=PV, seed=seed, dtype=torch.bfloat16)


def test_production_size_eval_runs_the_fused_stage1_and_survives_updates():
    """d=512, h=8, two layers, bf16, B=4, the default ladder, one ragged batch per frame-tile regime (T <= 32, 33..64, 65..128): the
    captured forward is the fused stage-1 inference launch (asserted through bist_launch_count around the capture), whose
    fragment-ordered W_v / W_o and the packed value projections exist only at this width -- so the weights-move sequence runs here once
    more.  The loss must move by more than three tolerances for that part to say anything (a result from the old weights would miss the
    bound by as much); six steps at factor 2, warm-up 20 raise the rate to 6e-3 on Xavier-scale weights."""
    import bist_amd.model as M
    from bist_amd import _lib
    from bist_amd import functional as Fn
    from bist_amd.data.classes import LengthClasses
    from bist_amd.train import Trainer
    args = _prod_args()
    Fn.manual_seed(1234)
    torch.manual_seed(0)
    model = M.make_model(PV, PV, args, ft_sizes=[PC]).cuda().train()
    t = Trainer(model, args, PV, compute_dtype=torch.bfloat16, warmup=20, factor=2.0, use_graph=True, length_classes=LengthClasses())
    ev = [_prod_batch(T, 500 + T) for T in (24, 50, 100)]
    assert len({t.length_classes.key(b) for b in ev}) == 3
    kw = dict(vocab=PV, feat=PC)
    ref = _eager_copy(model, args, torch.bfloat16, **kw)
    for b in ev:
        n0 = _lib.lib.bist_launch_count(_lib.K_ST1_FUSED)
        got = _floats(t.eval_step(b))                       # a capture: two warm-up passes and the recorded one
        grown = _lib.lib.bist_launch_count(_lib.K_ST1_FUSED) - n0
        assert grown >= 4, ("the fused stage-1 inference launch did not run", b.fts.shape, grown)
        _close(got, _eager_terms(ref, t, args, b), 2e-2, "T=%d" % b.fts.shape[1])
    del ref
    assert t.eval_graph_stats()["captures"] == 3
    steps = [_prod_batch(T, 600 + i) for i, T in enumerate((24, 50, 100, 24, 50, 100))]
    # two layers x attentions A1, A4 x (W_v, W_o) in fragment order; the fused launch projects the values itself: no packed projection
    _weights_move_graphs_stay(t, args, torch.bfloat16, ev, steps, 2e-2, 3, kw, (8, 0))
    print("eval entries: %s" % t.eval_graph_stats())
    # One dialogue: with the decoder's reasoning cache on, an inference forward of a single dialogue goes through the persistent
    # decode-step launch and its per-turn buffers (the yardstick below does); the evaluation path keeps to the layer-by-layer decoder.
    one = _prod_batch(24, 777, B=1)
    n0 = _lib.lib.bist_launch_count(_lib.K_DECSTACK)
    got = _floats(t.eval_step(one))
    assert _lib.lib.bist_launch_count(_lib.K_DECSTACK) == n0, "the evaluation step went through the decode-step launch"
    want = _eager_terms(_eager_copy(model, args, torch.bfloat16, **kw), t, args, one)
    print("decode-step launches in the eager yardstick of the one-dialogue batch: %d" % (_lib.lib.bist_launch_count(_lib.K_DECSTACK) - n0))
    _close(got, want, 2e-2, "one dialogue")
    assert "REASONING_CACHE" not in model.mutlimodal_decoder.__dict__ and type(model.mutlimodal_decoder).REASONING_CACHE is True
