"""Trainer checkpoints: snapshot / restore on the device, save / load through a file, at the small model sizes of
tests/test_deterministic_train_gpu.py (d = 64, h = 4, 2 + 2 + 2 layers, vocabulary 80, B = 4, T = 8, S = 9, C = 64).  Every trainer is
deterministic, and every comparison is torch.equal: a resumed or rolled-back run repeats the bits of the uninterrupted one."""
import argparse
import copy
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LADDER = {"query": (8, 16), "his": (8, 16), "cap": (8, 16), "trg": (8, 16), "frames": (8, 16)}
LADDER_STEPS = {"query": 8, "his": 8, "cap": 8, "trg": 8, "frames": 8}
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])


def _args(dropout=0.0):
    from oracle import bist_oracle as O
    cfg = O.Cfg(d_model=64, att_h=4, nb_blocks=2, nb_venc_blocks=2, nb_cenc_blocks=2, dropout=dropout)
    return argparse.Namespace(**{**cfg.__dict__, "d_ff": 4 * cfg.d_model})


def _trainer(dtype, dropout=0.0, seeds=(0, 7), **kw):
    """A deterministic trainer on a model built after torch.manual_seed(seeds[0]) and Fn.manual_seed(seeds[1])."""
    import bist_amd.model as M
    from bist_amd import functional as Fn
    from bist_amd.train import Trainer
    args = _args(dropout)
    torch.manual_seed(seeds[0])
    Fn.manual_seed(seeds[1])
    model = M.make_model(80, 80, args, ft_sizes=[64]).cuda()
    model.train(dropout > 0.0)
    return Trainer(model, args, 80, compute_dtype=dtype, warmup=20, factor=2.0, deterministic=True, **kw)


def _stranger(dtype, dropout=0.0, **kw):
    """The trainer a checkpoint is loaded into: other initial weights, another dropout seed."""
    return _trainer(dtype, dropout, seeds=(123, 99), **kw)


def _batch(seed, dtype, lo=8, hi=13, T=8, shape_seed=None):
    from bist_amd.data.synthetic import synthetic_batch
    rs = np.random.RandomState(seed if shape_seed is None else shape_seed)
    Lq, Lh, Lc, Lt = (int(rs.randint(lo, hi)) for _ in range(4))
    return synthetic_batch(4, T=T, S=9, C=64, Lq=Lq, Lh=Lh, Lc=Lc, Lt=Lt, vocab=80, seed=seed, dtype=dtype)


def _four(dtype):
    return [_batch(s, dtype, shape_seed=11) for s in (11, 12, 13, 14)]          # four different batches of one shape


def _classes():
    from bist_amd.data.classes import LengthClasses
    return LengthClasses(LADDER, LADDER_STEPS)


def _steps(tr, batches, group=False):
    terms = []
    for b in batches:
        out = tr.step_group(b) if group else tr.step(b)
        terms.append({k: v.clone() for k, v in out.items()})
    torch.cuda.synchronize()
    return terms


def _state(tr):
    torch.cuda.synchronize()
    return {"master": tr.master.clone(), "m": tr.m.clone(), "v": tr.v.clone(), "flat_param": tr.flat_param.clone()}


def _same_terms(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.keys() == y.keys()
        for k in x:
            assert torch.equal(x[k], y[k]), "%s: loss term %s of step %d: %r vs %r" % (what, k, i, x[k].item(), y[k].item())


def _same_state(a, b, what):
    for k in a:
        assert a[k].dtype == b[k].dtype
        assert torch.equal(a[k], b[k]), "%s: %s differs in %d elements" % (what, k, int((a[k] != b[k]).sum()))


# ---- 1. resume through a file -----------------------------------------------------------------------------------------------------------
def _resume(tmp_path, dtype, dropout, use_graph):
    batches = _four(dtype)
    a = _trainer(dtype, dropout, use_graph=use_graph)
    ta = _steps(a, batches)
    b = _trainer(dtype, dropout, use_graph=use_graph)
    _steps(b, batches[:2])
    path = str(tmp_path / "two_steps.pt")
    b.save(path)
    del b
    c = _stranger(dtype, dropout, use_graph=use_graph)
    assert not torch.equal(c.master, a.master)
    c.load(path)
    tc = _steps(c, batches[2:])
    assert c._step == 4
    _same_terms(ta[2:], tc, "uninterrupted vs resumed")
    _same_state(_state(a), _state(c), "uninterrupted vs resumed")
    assert (a.m != 0).any()


@DTYPES
def test_an_eager_run_with_dropout_resumes_from_a_file_bit_for_bit(tmp_path, dtype):
    _resume(tmp_path, dtype, 0.1, False)


@DTYPES
def test_a_replayed_run_without_dropout_resumes_from_a_file_bit_for_bit(tmp_path, dtype):
    _resume(tmp_path, dtype, 0.0, True)


# ---- 2. rollback in the process ---------------------------------------------------------------------------------------------------------
@DTYPES
def test_restore_repeats_the_steps_of_a_replayed_class_trainer_with_dropout(dtype):
    # classes "all 8", "all 16", "all 8" again, then a third one (tokens 8, frames 16) met only behind the snapshot
    shapes = [(31, 3, 9, 6), (32, 9, 14, 12), (33, 3, 9, 6), (34, 3, 9, 12)]
    batches = [_batch(s, dtype, lo, hi, T) for s, lo, hi, T in shapes]
    tr = _trainer(dtype, 0.1, use_graph=True, length_classes=_classes())
    _steps(tr, batches[:2])
    snap = tr.snapshot()
    at_snapshot = _state(tr)
    first = _steps(tr, batches[2:])
    after = _state(tr)
    captures = tr.graph_stats()["captures"]
    assert captures == 3 and tr._step == 4
    assert not torch.equal(after["master"], at_snapshot["master"])
    tr.restore(snap)
    assert tr._step == 2
    _same_state(_state(tr), at_snapshot, "restored vs snapshot time")            # flat_param: Adam's rounding of master
    assert tr.graph_stats()["captures"] == captures
    again = _steps(tr, batches[2:])
    _same_terms(first, again, "first time vs after restore")
    _same_state(after, _state(tr), "first time vs after restore")
    assert tr.graph_stats()["captures"] == captures and tr._step == 4


# ---- 3. options: accumulate and the non-finite guard ------------------------------------------------------------------------------------
def _with_inf(batch):
    bad = copy.copy(batch)
    bad.fts = batch.fts.clone()
    bad.fts.view(-1)[5] = float("inf")
    return bad


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "replay"])
def test_an_accumulating_clipping_trainer_resumes_with_its_counters(tmp_path, use_graph):
    dtype = torch.float32
    b = _four(dtype)
    groups = [[b[0], b[1]], [b[2], _with_inf(b[3])], [b[2], b[3]]]
    kw = dict(use_graph=use_graph, accumulate=True, max_grad_norm=math.inf)
    a = _trainer(dtype, **kw)
    ta = _steps(a, groups, group=True)
    assert a.clip_stats()["skipped"] == 1
    s = _trainer(dtype, **kw)
    _steps(s, groups[:2], group=True)
    sd = s.state_dict()
    assert sd["counters"] == {"step": 2, "passes": 4, "skipped": 1}
    path = str(tmp_path / "two_groups.pt")
    s.save(path)
    c = _stranger(dtype, **kw)
    c.load(path)
    assert c.clip_stats()["skipped"] == 1 and c._step == 2 and c._passes == 4
    tc = _steps(c, groups[2:], group=True)
    _same_terms(ta[2:], tc, "uninterrupted vs resumed group")
    _same_state(_state(a), _state(c), "uninterrupted vs resumed group")
    assert c.clip_stats() == a.clip_stats()


# ---- 4. what a snapshot holds, and what a file must hold ----------------------------------------------------------------------------------
def test_a_snapshot_holds_the_state_of_its_call_not_of_its_reading():
    dtype = torch.bfloat16
    b = _four(dtype)
    tr = _trainer(dtype)
    tr.step(b[0])
    snap = tr.snapshot()
    then = {k: getattr(tr, k).clone() for k in ("master", "m", "v")}             # (stream-ordered: before the next step's launches)
    tr.step(b[1])                                                                # queued before the snapshot is read
    sd = snap.state_dict()
    assert sd["counters"]["step"] == 1 and tr._step == 2
    for k in then:
        assert sd[k].device.type == "cpu" and torch.equal(sd[k], then[k].cpu()), k
        assert not torch.equal(getattr(tr, k), then[k]), k
    # into=: the same buffers, the later state
    again = tr.snapshot(into=snap)
    assert again is snap and torch.equal(snap.master, tr.master) and snap.step == 2
    from bist_amd.checkpoint import TrainerSnapshot
    with pytest.raises(ValueError, match="snapshot"):
        tr.snapshot(into=TrainerSnapshot(tr.numel - 64, tr.master.device, clip=False))
    with pytest.raises(ValueError, match="snapshot"):
        tr.restore(TrainerSnapshot(tr.numel + 64, tr.master.device, clip=False))


def test_a_flipped_bit_is_refused_by_the_digest_and_the_trainer_stays_as_it_was():
    dtype = torch.float32
    b = _four(dtype)
    tr = _trainer(dtype)
    _steps(tr, b[:2])
    sd = tr.state_dict()
    assert sd["digest"] == tr.state_digest()
    _steps(tr, b[2:3])
    before = _state(tr)
    sd["m"].view(torch.int32)[1234] ^= 1 << 3
    with pytest.raises(ValueError, match="digest"):
        tr.load_state_dict(sd)
    _same_state(before, _state(tr), "after the refused load")
    assert tr._step == 3
    sd["m"].view(torch.int32)[1234] ^= 1 << 3
    tr.load_state_dict(sd)
    assert tr._step == 2 and tr.state_digest() == sd["digest"]


def test_a_float32_checkpoint_loads_into_a_bfloat16_trainer(tmp_path):
    b = _four(torch.float32)
    src = _trainer(torch.float32)
    _steps(src, b[:2])
    path = str(tmp_path / "f32.pt")
    src.save(path)
    dst = _stranger(torch.bfloat16)
    dst.load(path)
    torch.cuda.synchronize()
    assert torch.equal(dst.master, src.master) and torch.equal(dst.m, src.m) and torch.equal(dst.v, src.v)
    assert dst.flat_param.dtype == torch.bfloat16 and torch.equal(dst.flat_param, dst.master.to(torch.bfloat16))
    for p, (_name, o, k, shape) in zip(dst.params, dst._layout):                 # the model's parameters are still views of flat_param
        assert p.data_ptr() == dst.flat_param.data_ptr() + 2 * o and tuple(p.shape) == shape


def test_evaluation_sees_the_restored_weights():
    dtype = torch.float32
    tr = _trainer(dtype, use_graph=True, length_classes=_classes())
    batches = [_batch(41, dtype, 3, 9, 6), _batch(42, dtype, 9, 14, 12), _batch(43, dtype, 3, 9, 6)]
    tr.step(batches[0])
    snap = tr.snapshot()
    first = tr.evaluate(batches)
    _steps(tr, batches[1:])
    moved = tr.evaluate(batches)
    assert moved != first
    captures = tr.eval_graph_stats()["captures"]
    tr.restore(snap)
    assert tr.evaluate(batches) == first
    assert tr.eval_graph_stats()["captures"] == captures


def test_state_digest_is_equal_after_equal_runs_and_moves_with_a_step():
    dtype = torch.bfloat16
    b = _four(dtype)
    x, y = _trainer(dtype), _trainer(dtype)
    _steps(x, b[:2])
    _steps(y, b[:2])
    dx = x.state_digest()
    assert set(dx) == {"master", "m", "v"} and all(isinstance(v, int) and 0 <= v < 2 ** 64 for v in dx.values())
    assert dx == y.state_digest()
    assert len(set(dx.values())) == 3
    _steps(y, b[2:3])
    dy = y.state_digest()
    assert all(dy[k] != dx[k] for k in dx)


# ---- 5. a trainer that exchanges gradients ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graphs", [True, False], ids=["two_graphs", "eager"])
def test_restore_on_an_exchanging_trainer_clears_the_bucket_flags(graphs):
    """The one-rank RCCL group of tests/test_train_gpu.py::test_exchange_path_matches_single_rank_step: the bucket flags in pinned memory
    carry step numbers, so going back in time must clear them -- else the first bucket of the repeated step 3 is exchanged at once."""
    import os, socket
    import torch.distributed as dist
    dtype = torch.float32
    b = _four(dtype)
    sock = socket.socket(); sock.bind(("127.0.0.1", 0)); port = sock.getsockname()[1]; sock.close()
    dist.init_process_group("nccl", rank=0, world_size=1, init_method=f"tcp://127.0.0.1:{port}", device_id=torch.device("cuda", 0))
    os.environ["BIST_FORCE_EXCHANGE"] = "1"
    try:
        tr = _trainer(dtype, use_graph=graphs)
        assert tr.exchanging and tr.overlap and not tr.adam_in_step
        _steps(tr, b[:2])
        snap = tr.snapshot()
        first = _steps(tr, b[2:])
        after = _state(tr)
        n = tr._flag_streams[0]
        assert n >= 1 and tr._flags[:n].tolist() == [4] * n
        tr.restore(snap)
        assert tr._flags.tolist() == [0] * tr._flags.numel() and tr._step == 2
        again = _steps(tr, b[2:])
        _same_terms(first, again, "first time vs after restore")
        _same_state(after, _state(tr), "first time vs after restore")
        n = tr._flag_streams[0]
        assert tr._flags[:n].tolist() == [4] * n
        other = tr.snapshot()
        other.config["world"] = 2
        with pytest.raises(ValueError, match="world"):
            tr.restore(other)
    finally:
        os.environ.pop("BIST_FORCE_EXCHANGE", None)
        dist.destroy_process_group()
