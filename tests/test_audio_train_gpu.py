"""Training with the audio modality through every Trainer mode, at the small model sizes of tests/test_deterministic_train_gpu.py plus two
audio reasoning layers (d_model 64, two blocks of each stack, audio features [B, Ta, 16]): captured steps, deterministic=True, length
classes with the audio rung (bist_stage_audio), evaluate(), step_group, max_grad_norm, save / load -- and the flat layout of a model
WITHOUT audio, which must be what it was before audio existed."""
import argparse
import copy
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LADDER = {"query": (8, 16), "his": (8, 16), "cap": (8, 16), "trg": (8, 16), "frames": (8, 16)}        # the audio ladder: the default one
LADDER_STEPS = {"query": 8, "his": 8, "cap": 8, "trg": 8, "frames": 8}
DA = 16
TERMS = ["out", "cap_ae", "audio_ae", "temporal_ae", "spatial_ae"]


def _args(dropout=0.0, audio=2, blocks=2):
    from oracle import bist_oracle as O
    cfg = O.Cfg(d_model=64, att_h=4, nb_blocks=blocks, nb_venc_blocks=blocks, nb_cenc_blocks=blocks, nb_aenc_blocks=audio, dropout=dropout)
    return argparse.Namespace(**{**cfg.__dict__, "d_ff": 4 * cfg.d_model})


def _trainer(dtype=torch.float32, dropout=0.0, deterministic=True, seeds=(0, 7), **kw):
    """A trainer on an audio model built after torch.manual_seed and Fn.manual_seed: the same weights and dropout seeds every time."""
    import bist_amd.model as M
    from bist_amd import functional as Fn
    from bist_amd.train import Trainer
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    args = _args(dropout)
    torch.manual_seed(seeds[0])
    Fn.manual_seed(seeds[1])
    model = M.make_model(80, 80, args, ft_sizes=[64, DA]).cuda()
    model.train(dropout > 0.0)
    return Trainer(model, args, 80, compute_dtype=dtype, warmup=20, factor=2.0, deterministic=deterministic, **kw)


def _batch(seed, dtype=torch.float32, lo=8, hi=13, T=8, Ta=9, shape_seed=None, B=4):
    from bist_amd.data.synthetic import synthetic_batch
    rs = np.random.RandomState(seed if shape_seed is None else shape_seed)
    Lq, Lh, Lc, Lt = (int(rs.randint(lo, hi)) for _ in range(4))
    return synthetic_batch(B, T=T, S=9, C=64, Lq=Lq, Lh=Lh, Lc=Lc, Lt=Lt, vocab=80, seed=seed, dtype=dtype, audio=(Ta, DA))


def _classes():
    from bist_amd.data.classes import LengthClasses
    return LengthClasses(LADDER, LADDER_STEPS)


def _run(tr, items, group=False):
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
        assert list(x) == list(y) == TERMS
        for k in x:
            assert torch.equal(x[k], y[k]), "%s: loss term %s of step %d: %r vs %r" % (what, k, i, x[k].item(), y[k].item())
    for name, x, y in zip(("master", "m", "v"), sa, sb):
        assert torch.equal(x, y), "%s: %s differs in %d elements" % (what, name, int((x != y).sum()))


def test_synthetic_audio_is_ragged_and_leaves_the_other_fields_alone():
    from bist_amd.data.synthetic import synthetic_batch
    kw = dict(T=8, S=9, C=64, Lq=9, Lh=10, Lc=8, Lt=9, vocab=80, seed=3, dtype=torch.float32)
    a, b = synthetic_batch(8, audio=(20, DA), **kw), synthetic_batch(8, **kw)
    for f in ("query", "his", "cap", "trg", "trg_y", "fts", "temporal_mask"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert b.audio_fts is None and tuple(a.audio_fts.shape) == (8, 20, DA) and tuple(a.audio_mask.shape) == (8, 1, 20)
    live = a.audio_mask.sum(-1).reshape(-1).tolist()
    assert max(live) == 20 and min(live) < 20 and min(live) >= 10, live


def test_three_eager_steps_against_three_replayed_steps_give_the_same_loss_terms():
    """LOSS TERMS only.  The bound of tests/test_train_gpu.py:530 (test_trainer_graph_replay_matches_eager: the loss of step i within 2e-3 (1 + i) of the
    eager run's, every term here) for the default, atomics-reordering trainers -- that test's reason: Adam turns rounding-level gradient
    differences of near-zero entries into full-size updates, so parameters are not comparable entry by entry there.  The parameters
    themselves are compared bit for bit under deterministic=True in the next test."""
    b = _batch(21)
    t1, t2 = _trainer(deterministic=False), _trainer(deterministic=False, use_graph=True)
    l1 = [{k: v.item() for k, v in t1.step(b).items()} for _ in range(3)]
    l2 = [{k: v.item() for k, v in t2.step(b).items()} for _ in range(3)]
    for i, (x, y) in enumerate(zip(l1, l2)):
        assert list(x) == list(y) == TERMS
        for k in x:
            assert abs(x[k] - y[k]) <= 2e-3 * (1 + i) * abs(x[k]), (i, k, x[k], y[k])
    assert l1[-1]["out"] < l1[0]["out"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_deterministic_runs_are_bit_identical_eager_replayed_and_twice(dtype):
    batches = [_batch(s, dtype, shape_seed=11) for s in (11, 12, 13)]
    eager = _run(_trainer(dtype), batches)
    replay = _run(_trainer(dtype, use_graph=True), batches)
    again = _run(_trainer(dtype, use_graph=True), batches)
    assert (eager[1] != 0).any()
    _same(eager, replay, "eager vs replay")
    _same(replay, again, "replay vs replay")


def test_deterministic_dropout_runs_are_bit_identical():
    runs = []
    for _ in range(2):
        tr = _trainer(torch.bfloat16, dropout=0.1, use_graph=True)
        runs.append(_run(tr, [_batch(s, torch.bfloat16, shape_seed=11) for s in (11, 12, 13)]))
        del tr
    _same(runs[0], runs[1], "run 1 vs run 2")


RAGGED = [(31, 9), (32, 20), (33, 33), (34, 9)]         # (seed, audio length): audio classes 16, 32, 48, 16


def test_class_mode_captures_one_graph_per_class_and_equals_the_exact_shape_replay():
    """Four ragged batches with audio lengths 9, 20, 33, 9 (token lengths and frames within one class): three classes, three captures,
    nothing captured in the second pass; every class step equals, bit for bit, the exact-shape replay of the padded batch it staged."""
    batches = [_batch(s, lo=9, hi=14, T=12, Ta=ta) for s, ta in RAGGED]
    lc = _classes()
    keys = [lc.key(b) for b in batches]
    assert len(set(keys)) == 3 and keys[0] == keys[3] and [k[11] for k in keys] == [16, 32, 48, 16]
    tc = _trainer(use_graph=True, length_classes=lc)
    tx = _trainer(use_graph=True)
    for i, b in enumerate(batches):
        a = tc.step(b)
        padded = copy.copy(tc._static_batch)
        for f in tc._BATCH_FIELDS:
            v = getattr(padded, f, None)
            if v is not None:
                setattr(padded, f, v.clone())
        assert padded.audio_fts.shape[1] == keys[i][11] and padded.audio_mask.shape == (4, 1, keys[i][11])
        assert torch.equal(padded.audio_mask[:, :, :b.audio_fts.shape[1]], b.audio_mask) and not padded.audio_mask[:, :, b.audio_fts.shape[1]:].any()
        c = tx.step(padded)
        torch.cuda.synchronize()
        assert list(a) == TERMS
        for k in a:
            assert torch.equal(a[k], c[k]), (i, k)
        assert torch.equal(tc.flat_grad, tx.flat_grad), "step %d: %d gradient elements differ" % (i, int((tc.flat_grad != tx.flat_grad).sum()))
        assert torch.equal(tc.master, tx.master), i
    st = tc.graph_stats()
    assert st["captures"] == 3 and st["hits"] == 1, st
    for b in batches:
        tc.step(b)
    st = tc.graph_stats()
    assert st["captures"] == 3 and st["hits"] == 5, st


def _eager_eval(tr, args, batches):
    """run_epoch(..., eval=True)'s arithmetic on a fresh eager model with the trainer's present weights: eval(), no_grad, forward,
    SimpleLossCompute.terms per batch; un-normalised sums over summed token counts (train.py:32-37, 49-51)."""
    import bist_amd.model as M
    from bist_amd.model.optimize import SimpleLossCompute
    fresh = M.make_model(80, 80, args, ft_sizes=[64, DA])
    sd = {k: v.detach().float().cpu() for k, v in tr.model.state_dict().items()}
    missing, unexpected = fresh.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith(".pe") for k in missing)
    fresh = fresh.cuda().eval()
    lc = SimpleLossCompute(fresh.generator, fresh.ae_generator, tr.criterion, opt=None, args=args)
    tot, tok, qtok = {}, 0, 0
    with torch.no_grad():
        for b in batches:
            terms, _ = lc.terms(fresh.forward(b), b)
            n, q = int(b.ntokens.item()), int(b.qntokens.item())
            for k, v in terms.items():
                tot[k] = tot.get(k, 0.0) + v.double().item() * (n if k == "out" else q)
            tok, qtok = tok + n, qtok + q
    return {k: v / (tok if k == "out" else qtok) for k, v in tot.items()}, tok, qtok


def test_evaluate_returns_all_five_terms_equal_to_the_eager_epoch():
    """The fp32 bound of tests/test_eval_classes_gpu.py:27-28, 144 (class evaluation against the eager evaluation: 1e-5 relative per term)."""
    TOL32 = 1e-5
    tr = _trainer(use_graph=True, length_classes=_classes())
    batches = [_batch(s, lo=9, hi=14, T=12, Ta=ta) for s, ta in RAGGED]
    tr.step(batches[0])
    got = tr.evaluate(batches)
    want, tok, qtok = _eager_eval(tr, _args(), batches)
    assert set(TERMS) <= set(got) and list(want) == TERMS
    for k in TERMS:
        print("evaluate %s: got %.9g want %.9g rel %.3e" % (k, got[k], want[k], abs(got[k] - want[k]) / abs(want[k])))
    for k in TERMS:
        assert abs(got[k] - want[k]) <= TOL32 * abs(want[k]), (k, got[k], want[k])
    assert got["tokens"] == tok and got["qtokens"] == qtok and got["batches"] == 4
    st = tr.eval_graph_stats()
    assert st["captures"] == 3 and st["hits"] == 1, st


def _select(batch, idx):
    from bist_amd.data.batch import Batch
    idx = torch.as_tensor(idx, device=batch.query.device)
    return Batch(batch.query[idx], batch.his[idx], batch.fts[idx], batch.cap[idx], batch.trg[idx], batch.trg_y[idx],
                 audio_fts=[batch.audio_fts[idx]])


def test_a_group_of_two_batches_is_the_step_on_their_union():
    """The f32 bound of tests/test_accumulate_train_gpu.py:139-141: per piece the first moment within 2e-4 of its largest entry, the loss
    terms within 1e-5."""
    full = _batch(51, lo=12, hi=13)
    h0, h1 = _select(full, [0, 1]), _select(full, [2, 3])
    full = _select(full, [0, 1, 2, 3])
    tg, tf = _trainer(accumulate=True), _trainer()
    a = tg.step_group([h0, h1])
    c = tf.step(full)
    torch.cuda.synchronize()
    assert list(a) == list(c) == TERMS
    for lo, hi in tf.pieces:
        scale, err = tf.m[lo:hi].abs().max().item(), (tg.m[lo:hi] - tf.m[lo:hi]).abs().max().item()
        assert scale > 0 and err <= 2e-4 * scale, (lo, hi, err, scale)
    for k in a:
        assert abs(a[k].item() - c[k].item()) <= 1e-5 * abs(c[k].item()), (k, a[k].item(), c[k].item())


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "replay"])
def test_an_infinite_clipping_bound_is_the_plain_trainer_bit_for_bit(use_graph):
    batches = [_batch(s, torch.bfloat16, shape_seed=11) for s in (11, 12, 13)]
    plain = _run(_trainer(torch.bfloat16, dropout=0.1, use_graph=use_graph), batches)
    clip = _run(_trainer(torch.bfloat16, dropout=0.1, use_graph=use_graph, max_grad_norm=math.inf), batches)
    _same(plain, clip, "plain vs max_grad_norm=inf")


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "replay"])
def test_save_load_one_step_equals_the_uninterrupted_run(tmp_path, use_graph):
    batches = [_batch(s, shape_seed=11) for s in (11, 12, 13)]
    a = _trainer(use_graph=use_graph)
    ta = _run(a, batches)
    b = _trainer(use_graph=use_graph)
    _run(b, batches[:2])
    path = str(tmp_path / "audio_two_steps.pt")
    b.save(path)
    del b
    c = _trainer(use_graph=use_graph, seeds=(123, 99))
    assert not torch.equal(c.master, a.master)
    c.load(path)
    tc = _run(c, batches[2:])
    assert c._step == 3
    _same((ta[0][2:],) + ta[1:], tc, "uninterrupted vs resumed")
    msd = c.master_state_dict()
    assert any(".a_layers.1." in k for k in msd) and "vid_encoder.a_W.weight" in msd
    assert all(v.dtype == torch.float32 for v in msd.values())


def test_restore_repeats_the_steps_behind_a_snapshot_bit_for_bit():
    batches = [_batch(s, shape_seed=11) for s in (11, 12, 13)]
    tr = _trainer(use_graph=True)
    tr.step(batches[0])
    snap = tr.snapshot()
    first = _run(tr, batches[1:])
    tr.restore(snap)
    assert tr._step == 1
    second = _run(tr, batches[1:])
    _same(first, second, "before vs after restore")


def _host(seed, Ta, as_list):
    from bist_amd.data.feeder import HostBatch
    b = _batch(seed, torch.float32, lo=9, hi=14, T=12, Ta=Ta)
    cpu = lambda t: t.cpu()
    au = cpu(b.audio_fts)
    return HostBatch(cpu(b.query), cpu(b.his), cpu(b.fts), cpu(b.cap), cpu(b.trg), cpu(b.trg_y), audio_fts=[au.numpy()] if as_list else au)


def test_a_fed_class_step_with_f32_host_audio_equals_the_resident_step():
    """DeviceFeeder(length_classes=...): f32 HostBatch audio (once as the reference's list of one array) crosses in its slot in the
    source dtype, arrives as a SourceBatch whose audio_mask is derived on first access only, and a bf16 class-mode trainer stages and
    casts it (bist_stage_audio): the step is the resident step bit for bit under deterministic=True -- the same launches on the same
    values.  Slots are reused from the fourth batch on."""
    from bist_amd.data.batch import Batch, SourceBatch
    from bist_amd.data.feeder import DeviceFeeder
    lc = _classes()
    hosts = [_host(71 + i, ta, i % 2 == 0) for i, ta in enumerate((9, 20, 9, 33, 20))]
    t1 = _trainer(torch.bfloat16, use_graph=True, length_classes=lc)
    t2 = _trainer(torch.bfloat16, use_graph=True, length_classes=lc)
    for i, (hb, fb) in enumerate(zip(hosts, DeviceFeeder(hosts, length_classes=lc))):
        assert isinstance(fb, SourceBatch) and fb.audio_fts.is_cuda and fb.audio_fts.dtype == torch.float32
        assert torch.equal(fb.audio_fts.cpu(), hb.audio_fts) and "audio_mask" not in fb.__dict__
        a = t1.step(fb)
        rb = Batch(hb.query.cuda(), hb.his.cuda(), hb.fts.cuda(), hb.cap.cuda(), hb.trg.cuda(), hb.trg_y.cuda(), audio_fts=hb.audio_fts.cuda())
        assert torch.equal(fb.audio_mask, rb.audio_mask)
        c = t2.step(rb)
        torch.cuda.synchronize()
        assert list(a) == TERMS
        for k in a:
            assert torch.equal(a[k], c[k]), (i, k)
        assert torch.equal(t1.flat_grad, t2.flat_grad) and torch.equal(t1.master, t2.master), i
        assert t1._static_batch.audio_fts.dtype == torch.bfloat16
    assert t1.graph_stats()["captures"] == 3


def test_the_feeder_without_classes_casts_audio_like_the_video_features():
    from bist_amd.data.feeder import DeviceFeeder
    hosts = [_host(81 + i, 9, i == 0) for i in range(4)]
    for hb, fb in zip(hosts, DeviceFeeder(hosts, feature_dtype=torch.bfloat16)):
        assert fb.audio_fts.dtype == torch.bfloat16 == fb.fts.dtype and tuple(fb.audio_fts.shape) == tuple(hb.audio_fts.shape)
        assert torch.equal(fb.audio_fts.cpu(), hb.audio_fts.to(torch.bfloat16)) and torch.equal(fb.fts.cpu(), hb.fts.to(torch.bfloat16))
        assert torch.equal(fb.audio_mask.cpu(), (hb.audio_fts.to(torch.bfloat16).float().sum(-1) != 0).unsqueeze(-2))


def test_audio_layers_lie_in_the_pieces_of_their_blocks():
    tr = _trainer()
    names = {id(p): n for n, p in tr.model.named_parameters()}
    assert len(tr.pieces) == 1 + 1 + 2 and tr.pieces[-1][1] == tr.numel
    assert all(x[1] == y[0] for x, y in zip(tr.pieces, tr.pieces[1:])) and tr.pieces[0][0] == 0       # contiguous ranges
    for p in tr.params:
        n = names[id(p)]
        if ".a_layers." in n and p.dim() == 2:
            l = int(n.split(".a_layers.")[1].split(".")[0])
            off = p._grad_view.data_ptr() - tr.flat_grad.data_ptr()
            lo, hi = tr.pieces[2 + l]
            assert lo <= off // tr.flat_grad.element_size() < hi, (n, off, lo, hi)


def test_a_model_without_audio_keeps_its_flat_layout():
    """numel, pieces and buckets of the no-audio model, recorded from the commit before audio with the same construction
    (tests/test_audio_train_gpu.py's _trainer with nb_aenc_blocks = 0, two and six blocks, use_graph=True)."""
    import bist_amd.model as M
    from bist_amd.train import Trainer
    want = {2: (713408, [(0, 19648), (19648, 58048), (58048, 385728), (385728, 713408)]),
            6: (2049728, [(0, 45248), (45248, 83648), (83648, 411328), (411328, 739008), (739008, 1066688), (1066688, 1394368),
                          (1394368, 1722048), (1722048, 2049728)])}
    for blocks, (numel, pieces) in want.items():
        args = _args(audio=0, blocks=blocks)
        torch.manual_seed(0)
        tr = Trainer(M.make_model(80, 80, args, ft_sizes=[64]).cuda(), args, 80, compute_dtype=torch.float32, use_graph=True)
        assert tr.numel == numel and tr.pieces == pieces, (blocks, tr.numel, tr.pieces)
        assert tr.buckets == BUCKETS_BEFORE[blocks], (blocks, tr.buckets)
        assert tr._term_names() == ["out", "cap_ae", "temporal_ae", "spatial_ae"]


BUCKETS_BEFORE = {2: [(1, 385728, 713408)], 6: [(4, 1394368, 2049728), (2, 739008, 1394368)]}
