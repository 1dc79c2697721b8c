"""Training on ragged batches with length classes (Trainer(length_classes=...)): one captured step per class in a bounded store, each
batch staged into its class's static batch by bist_stage_train_batch.  Checked against eager steps on the SAME batches unpadded, at the
small model sizes of the other Trainer tests, dropout off: loss terms and the gradient each replay leaves in ``flat_grad``, replays of
several classes interleaved, evictions, a six-step training run, and the several-rank step (two gloo processes on one GPU)."""
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


def _args():
    from oracle import bist_oracle as O
    cfg = O.Cfg(d_model=64, att_h=4, nb_blocks=2, nb_venc_blocks=2, nb_cenc_blocks=2)
    return argparse.Namespace(**{**cfg.__dict__, "d_ff": 4 * cfg.d_model})


def _model(args):
    import bist_amd.model as M
    torch.manual_seed(0)
    return M.make_model(80, 80, args, ft_sizes=[64]).cuda().eval()


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


def _cos(a, b):
    a, b = a.double(), b.double()
    return (a @ b / (a.norm() * b.norm()).clamp_min(1e-30)).item()


def _pair(dtype, max_graphs=8, factor=0.0, warmup=20):
    """A class-mode graph trainer and an eager trainer from the same weights (factor 0: the weights never move, so every step is compared
    at the same point)."""
    from bist_amd.train import Trainer
    args = _args()
    m1 = _model(args)
    m2 = copy.deepcopy(m1)
    tg = Trainer(m1, args, 80, compute_dtype=dtype, warmup=warmup, factor=factor, use_graph=True, length_classes=_classes(),
                 max_graphs=max_graphs)
    te = Trainer(m2, args, 80, compute_dtype=dtype, warmup=warmup, factor=factor)
    return tg, te


def _compare_steps(tg, te, seq, dtype):
    worst_ee, worst_ge, worst_cos = 0.0, 0.0, 1.0
    for cls, seed in seq:
        b = _batch(cls, seed, dtype)
        tg_terms = tg.step(b)
        g_graph = tg.flat_grad.clone()
        te_terms = te.step(b)
        g_eager = te.flat_grad.clone()
        te.backward(b)                                  # the same eager gradient once more: the run-to-run spread of the fp32 atomics
        g_eager2 = te.flat_grad.clone()
        torch.cuda.synchronize()
        for k in te_terms:
            a, c = tg_terms[k].double().item(), te_terms[k].double().item()
            tol = 1e-5 if dtype == torch.float32 else 2e-2
            assert abs(a - c) <= tol * abs(c), (cls, seed, k, a, c)
        worst_ee = max(worst_ee, _rel(g_eager2, g_eager))
        worst_ge = max(worst_ge, _rel(g_graph, g_eager))
        worst_cos = min(worst_cos, _cos(g_graph, g_eager))
    print("gradient: graph vs eager rel %.3e, eager vs eager rel %.3e, cosine %.6f" % (worst_ge, worst_ee, worst_cos))
    if dtype == torch.float32:
        assert worst_ge <= max(10 * worst_ee, 1e-6), (worst_ge, worst_ee)
    else:
        assert worst_cos >= 0.995, worst_cos
    return worst_ge, worst_ee


SEQ12 = [("A", 11), ("B", 12), ("A", 13), ("B", 14), ("C", 15), ("A", 16), ("C", 17), ("B", 18), ("C", 19), ("A", 20), ("B", 21), ("C", 22)]


def test_ragged_sequence_captures_once_per_class_and_matches_eager():
    from bist_amd.data.classes import LengthClasses
    tg, te = _pair(torch.float32)
    lc = _classes()
    assert len({lc.key(_batch(c, s)) for c, s in SEQ12}) == 3
    assert len({LengthClasses.lengths(_batch(c, s))["query"] for c, s in SEQ12}) > 3      # ragged: many exact shapes
    _compare_steps(tg, te, SEQ12, torch.float32)          # starts A, B, A, B: replays of two class graphs interleaved
    st = tg.graph_stats()
    assert st["captures"] == 3 and st["hits"] == 9 and st["evictions"] == 0 and st["entries"] == 3, st
    assert st["bytes"] > 0


def test_evictions_keep_the_results():
    tg, te = _pair(torch.float32, max_graphs=2)
    _compare_steps(tg, te, SEQ12[:8], torch.float32)
    st = tg.graph_stats()
    # A B A B C A C B with room for two: C evicts A, A evicts B, B evicts A
    assert st["entries"] == 2 and st["evictions"] == 3 and st["captures"] == 5 and st["hits"] == 3, st


def test_bf16_gradients_of_padded_replays():
    tg, te = _pair(torch.bfloat16)
    _compare_steps(tg, te, SEQ12[:6], torch.bfloat16)
    assert tg.graph_stats()["captures"] == 3


def test_six_steps_with_classes_track_eager_training():
    """The drift bound of test_trainer_graph_replay_matches_eager (tests/test_train_gpu.py)."""
    tg, te = _pair(torch.float32, factor=2.0)
    seq = SEQ12[:6]
    l1, l2 = [], []
    for cls, seed in seq:
        b = _batch(cls, seed)
        l1.append(te.step(b)["out"].item())
        l2.append(tg.step(b)["out"].item())
    assert all(abs(a - c) <= 2e-3 * (1 + i) * abs(a) for i, (a, c) in enumerate(zip(l1, l2))), (l1, l2)
    assert tg.graph_stats()["captures"] == 3          # A B A B C A


def _deferred_run(seq):
    """An eager trainer and a class-mode graph trainer with the deferred optimiser (the update of step t applied at the head of step
    t+1) over `seq`, from the same weights -> (eager losses, deferred losses, eager model, deferred model, initial parameters, trainer)."""
    from bist_amd.train import Trainer
    args = _args()
    m1 = _model(args)
    m2 = copy.deepcopy(m1)
    p0 = {k: v.detach().clone() for k, v in m1.named_parameters()}
    te = Trainer(m1, args, 80, compute_dtype=torch.float32, warmup=20, factor=2.0)
    td = Trainer(m2, args, 80, compute_dtype=torch.float32, warmup=20, factor=2.0, use_graph=True, length_classes=_classes(),
                 deferred_adam=True)
    assert td.deferred
    l1, l2 = [], []
    for cls, seed in seq:
        b = _batch(cls, seed)
        l1.append(te.step(b)["out"].item())
        l2.append(td.step(b)["out"].item())
    td.flush()
    torch.cuda.synchronize()
    return l1, l2, m1, m2, p0, td


def _weights_apart(m1, m2, p0):
    """|w_deferred - w_eager| / |w_eager - w_initial| over the parameters (key-projection biases left out: their gradient is exactly
    zero -- softmax is shift invariant -- so Adam turns rounding noise into full-size steps of random sign in both runs)."""
    p1, p2 = dict(m1.named_parameters()), dict(m2.named_parameters())
    keys = [k for k in p1 if not k.endswith("linears.1.bias")]
    apart = sum(((p2[k].detach() - p1[k].detach()).double() ** 2).sum().item() for k in keys) ** 0.5
    moved = sum(((p1[k].detach() - p0[k]).double() ** 2).sum().item() for k in keys) ** 0.5
    return apart / moved


DEFERRED_SEQ = [("A", 31), ("B", 32), ("A", 33), ("C", 34), ("B", 35)]


def test_deferred_optimiser_keeps_every_update_across_class_captures():
    """The captures of classes B (step 2) and C (step 4) happen while an update is pending: it is applied before their warm-up passes
    overwrite the gradient it reads, so no step's gradient is lost."""
    l1, l2, m1, m2, p0, td = _deferred_run(DEFERRED_SEQ)
    assert td.graph_stats()["captures"] == 3
    print("losses eager %s deferred %s; weights apart / moved %.3e" % (l1, l2, _weights_apart(m1, m2, p0)))
    assert all(abs(a - c) <= 2e-3 * (1 + i) * abs(a) for i, (a, c) in enumerate(zip(l1, l2))), (l1, l2)
    assert _weights_apart(m1, m2, p0) <= 0.1
    assert int(td.pending.item()) == 0


def test_class_trainer_takes_sliced_features():
    """Features sliced out of a longer tensor (not contiguous): staged through a contiguous copy, the same step as the contiguous batch."""
    tg, te = _pair(torch.float32)
    b = _batch("A", 41)
    wide = torch.zeros(b.fts.shape[0], b.fts.shape[1] + 3, *b.fts.shape[2:], device="cuda")
    wide[:, :b.fts.shape[1]] = b.fts
    sl = copy.copy(b)
    sl.fts = wide[:, :b.fts.shape[1]]
    assert not sl.fts.is_contiguous()
    a = tg.step(sl)
    g_sl = tg.flat_grad.clone()
    c = te.step(b)
    torch.cuda.synchronize()
    for k in c:
        assert abs(a[k].item() - c[k].item()) <= 1e-5 * abs(c[k].item()), k
    assert _rel(g_sl, te.flat_grad) <= 1e-6


def test_default_trainer_keeps_one_exact_shape_graph():
    """Without length classes: one graph keyed by the exact shape (the store stays empty)."""
    from bist_amd.data.synthetic import synthetic_batch
    from bist_amd.train import Trainer
    args = _args()
    t = Trainer(_model(args), args, 80, compute_dtype=torch.float32, warmup=20, factor=2.0, use_graph=True)
    b = synthetic_batch(4, T=6, S=9, C=64, Lq=7, Lh=9, Lc=6, Lt=6, vocab=80, dtype=torch.float32)
    for _ in range(2):
        t.step(b)
    torch.cuda.synchronize()
    assert t.graph_stats()["captures"] == 0 and t.graph_stats()["entries"] == 0
    assert tuple(t._static_batch.query.shape) == (4, 7)


# ---- several ranks ----------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _worker(rank, world, port, q):
    import torch.distributed as dist
    from bist_amd import functional as Fn
    from bist_amd.train import Trainer
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    args = _args()
    t = Trainer(_model(args), args, 80, compute_dtype=torch.float32, warmup=20, factor=2.0, use_graph=True, length_classes=_classes())
    assert t.exchanging and not t.adam_in_step and t.world == world
    seen, checks = set(), []
    orig = Fn.Graph.replay

    def replay(g):
        if id(g) not in seen and g is t._graph:       # the first replay of a newly captured class graph
            seen.add(id(g))
            checks.append((t._flags_np.copy().tolist() if t._flags_np is not None else None, t._step))
        return orig(g)
    Fn.Graph.replay = replay
    try:
        for cls, seed in (("A", 200 + rank), ("C", 300 + rank)):          # two ragged steps, a new class each (per rank: its own shard)
            t.step(_batch(cls, seed))
    finally:
        Fn.Graph.replay = orig
    torch.cuda.synchronize()
    q.put((rank, t.master.cpu().numpy(), checks, bool(t.overlap), t.graph_stats()))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_with_classes_wait_for_the_replay_and_agree():
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = {}
    for _ in range(world):
        r, master, checks, overlap, stats = q.get(timeout=300)
        got[r] = (master, checks, overlap, stats)
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for r, (_, checks, overlap, stats) in got.items():
        assert overlap, "the overlapped exchange (bucket flags) is what this test checks"
        assert stats["captures"] == 2 and len(checks) == 2, (r, stats, checks)
        for flags, step in checks:              # right before the first replay of a new class graph: every flag below the step number
            assert all(f < step for f in flags), (r, flags, step)
    assert np.array_equal(got[0][0], got[1][0]), "ranks diverged"
