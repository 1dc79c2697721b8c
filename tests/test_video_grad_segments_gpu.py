"""The video tensor's gradient through FanOutFn's sink (BIST_VIDEO_GRAD_SEG=1): the score terms dsc^T.Qf and the value terms dV.W_v of
all reasoning layers are left as segments and formed by one bist_gemm_kseg launch per operand layout, instead of one product per term
and a bist_add_n over the results.  Switch 0 and switch 1 are compared IN ONE PROCESS (the switch is read per backward node) on the
gradient of the video tensor and of the input projection P0 behind it, eager and replayed; plus the reference's golden gradients, run-to
-run bits under Trainer(deterministic=True), the model variants that change who produces a term, the launch counters, and the failure
of a re-wrapped placeholder.

Bounds: f32 F32_TOL = 2e-5 and bf16 BF16_TOL = 1.2e-2, times max(1, |ref|max) as in tests/test_gemm_fine_tile_gpu.py::_cmp (the two
forms differ by where the sum of the terms is rounded); replay against eager 2e-4 of the largest entry in f32, the bound of
tests/test_train_gpu.py::test_replayed_and_deferred_steps_track_the_eager_run_parameter_for_parameter."""
import argparse
import copy
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import bist_oracle as O

pytestmark = pytest.mark.gpu

F32_TOL = 2e-5
BF16_TOL = 1.2e-2
SWITCH = "BIST_VIDEO_GRAD_SEG"


def _args(cfg):
    return argparse.Namespace(**{**cfg.__dict__, "d_ff": 4 * cfg.d_model})


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    import bist_amd.model as M
    from bist_amd import _lib
    assert _lib.lib.bist_device_ok() == 1, _lib.lib.bist_last_error()
    return M


def _cmp(got, ref, tol, what):
    """the project's bound, and -- because gradients are far below 1, where that bound alone would pass a missing term -- the direction:
    rounding differences of relative size e per element leave the cosine above 1 - 2 e^2 (f32: e ~ 24 * 2^-24, bf16: e ~ 2 * 2^-9 * the
    ratio of the largest term to the sum, taken as 3), a missing term of 24 does not"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    err = (got - ref).abs().max().item()
    scale = max(1.0, ref.abs().max().item())
    assert math.isfinite(err) and err <= tol * scale, f"{what}: max err {err:.3e} (scale {scale:.3e}, tol {tol})"
    cos = torch.nn.functional.cosine_similarity(got.flatten(), ref.flatten(), dim=0).item()
    assert cos >= (1 - 1e-8 if tol == F32_TOL else 1 - 3e-4), f"{what}: cosine {cos:.10f}"


# name -> (Cfg arguments, (B, T, S, Lq), dtype, audio layers): rows per clip T*S below 128, exactly 128 and above 128 all occur
MODELS = {
    "small_f32": (dict(d_model=128, att_h=2), (2, 5, 9, 7), torch.float32),
    "ts128_f32": (dict(d_model=128, att_h=2), (2, 8, 16, 7), torch.float32),
    "fused_bf16": (dict(d_model=512, att_h=8), (1, 32, 49, 20), torch.bfloat16),
    "t64_bf16": (dict(d_model=512, att_h=8), (1, 64, 9, 7), torch.bfloat16),
    "one_direction_f32": (dict(d_model=128, att_h=2, s2t=0), (2, 5, 9, 7), torch.float32),
    "audio_f32": (dict(d_model=128, att_h=2, nb_aenc_blocks=2), (2, 5, 9, 7), torch.float32),
}
_CACHE = {}


def _setup(M, name):
    """(args, model on the device, batch) of a variant; built once per module and never modified (users deep-copy the model)"""
    if name not in _CACHE:
        from bist_amd.data.synthetic import synthetic_batch
        kw, (B, T, S, Lq), dtype = MODELS[name]
        cfg = O.Cfg(nb_blocks=2, nb_venc_blocks=2, nb_cenc_blocks=2, **kw)
        args = _args(cfg)
        torch.manual_seed(0)
        audio = cfg.nb_aenc_blocks > 0
        model = M.make_model(80, 80, args, ft_sizes=[64, 16] if audio else [64]).cuda().to(dtype).eval()
        b = synthetic_batch(B, T=T, S=S, C=64, Lq=Lq, Lh=9, Lc=6, Lt=6, vocab=80, dtype=dtype, **(dict(audio=(10, 16)) if audio else {}))
        _CACHE[name] = (args, model, b)
    return _CACHE[name]


def _autograd_grads(M, name, switch, monkeypatch):
    """plain autograd (no trainer): -> (gradient of the video tensor, gradient of P0's weight, launch counts)"""
    from bist_amd import _lib
    from bist_amd.model.label_smoothing import LabelSmoothing
    from bist_amd.model.optimize import SimpleLossCompute
    args, model0, b = _setup(M, name)
    model = copy.deepcopy(model0)
    monkeypatch.setenv(SWITCH, str(switch))
    seen = {}

    def hook(_mod, _inp, out):
        out["spatiotemporal_ft"].register_hook(lambda g: seen.__setitem__("vft", g.detach().clone()))
    h = model.vid_encoder.register_forward_hook(hook)
    try:
        lc = SimpleLossCompute(model.generator, model.ae_generator, LabelSmoothing(80, O.PAD_ID, 0.1), None, args=args)
        terms, _ = lc.terms(model.forward(b), b)
        _lib.lib.bist_launch_count_reset()
        sum(terms.values()).backward()
        torch.cuda.synchronize()
    finally:
        h.remove()
    counts = (_lib.lib.bist_launch_count(_lib.K_GEMM_KSEG), _lib.lib.bist_launch_count(_lib.K_ADD_N))
    return seen["vft"], model.vid_encoder.W.weight.grad.detach().clone(), counts


@pytest.mark.parametrize("name", list(MODELS))
def test_switch_on_equals_switch_off_under_autograd(hip, monkeypatch, name):
    tol = F32_TOL if MODELS[name][2] == torch.float32 else BF16_TOL
    v0, w0, c0 = _autograd_grads(hip, name, 0, monkeypatch)
    v1, w1, c1 = _autograd_grads(hip, name, 1, monkeypatch)
    print(f"{name}: |dvft| {v0.abs().max().item():.3e} diff {(v1.double() - v0.double()).abs().max().item():.3e}; "
          f"|dW| {w0.abs().max().item():.3e} diff {(w1.double() - w0.double()).abs().max().item():.3e}; kseg/add_n launches off {c0} on {c1}")
    _cmp(v1, v0, tol, "gradient of the video tensor")
    _cmp(w1, w0, tol, "gradient of P0's weight")
    assert c0[0] == 0, "switch 0 must not use the K-segmented kernel"
    if name != "one_direction_f32":              # (one direction: its value projection is not a leaf product -- every term a tensor, as before)
        assert c1[0] >= 1 and c1[1] <= c0[1], (c0, c1)


def test_launch_counts_of_the_fused_training_step(hip, monkeypatch):
    """two layers, both directions, fused stage 1 (own values for neither direction at T = 32): 4 score terms and 4 value terms -- 8
    products and one 8-term bist_add_n become two K-segmented launches; the video tensor's fan calls bist_add_n no more"""
    _, _, c0 = _autograd_grads(hip, "fused_bf16", 0, monkeypatch)
    _, _, c1 = _autograd_grads(hip, "fused_bf16", 1, monkeypatch)
    assert c0[0] == 0 and c1[0] == 2, (c0, c1)
    assert c1[1] == c0[1] - 1, (c0, c1)


@pytest.mark.parametrize("own_v", [1, 2])
def test_own_value_modes(hip, monkeypatch, own_v):
    """BIST_FUSED_TRAIN_OWN_V = 1 / 2: the fused launch projects the values of both / of the s2t direction, and the value terms come
    from St1FusedTrainFn's own_v branch instead of the leaf projection"""
    from bist_amd import functional as Fn
    monkeypatch.setattr(Fn, "FUSED_TRAIN_OWN_V", own_v)
    v0, w0, c0 = _autograd_grads(hip, "fused_bf16", 0, monkeypatch)
    v1, w1, c1 = _autograd_grads(hip, "fused_bf16", 1, monkeypatch)
    _cmp(v1, v0, BF16_TOL, "gradient of the video tensor")
    _cmp(w1, w0, BF16_TOL, "gradient of P0's weight")
    assert c0[0] == 0 and c1[0] == 2, (c0, c1)


def _trainer_grad(M, name, switch, monkeypatch, steps=1, split=True, **kw):
    """Flat gradients of a trainer's passes over the variant's batch.  The optimiser runs OUTSIDE the step (BIST_ADAM_IN_STEP=0), so
    that a captured step leaves its gradient in flat_grad: an eager trainer runs backward(), a replaying one step() -- whose first
    call captures and then REPLAYS, at the initial weights.  split: the split executor, or the runtime's own graph executor."""
    from bist_amd import train
    args, model0, b = _setup(M, name)
    monkeypatch.setenv(SWITCH, str(switch))
    monkeypatch.setenv("BIST_ADAM_IN_STEP", "0")
    monkeypatch.setattr(train, "SPLIT_GRAPH", bool(split))
    model = copy.deepcopy(model0)
    tr = train.Trainer(model, args, 80, compute_dtype=MODELS[name][2], warmup=20, factor=2.0, **kw)
    w = model.vid_encoder.W.weight
    grads = []
    for _ in range(steps):
        tr.step(b) if kw.get("use_graph") else tr.backward(b)
        torch.cuda.synchronize()
        grads.append((tr.flat_grad.detach().clone(), w._grad_view.detach().clone()))
    return grads


@pytest.mark.parametrize("split", [True, False], ids=["split_executor", "runtime_executor"])
@pytest.mark.parametrize("name", ["small_f32", "fused_bf16"])
def test_replayed_step_equals_the_eager_step_with_either_switch(hip, monkeypatch, name, split):
    f32 = MODELS[name][2] == torch.float32
    tol = F32_TOL if f32 else BF16_TOL
    e0 = _trainer_grad(hip, name, 0, monkeypatch, use_graph=False)[-1]
    e1 = _trainer_grad(hip, name, 1, monkeypatch, use_graph=False)[-1]
    g0 = _trainer_grad(hip, name, 0, monkeypatch, use_graph=True, split=split)[-1]
    g1 = _trainer_grad(hip, name, 1, monkeypatch, use_graph=True, split=split)[-1]
    assert e1[0].abs().max().item() > 0 and g1[0].abs().max().item() > 0
    _cmp(e1[1], e0[1], tol, "eager: P0's flat gradient, switch 1 against 0")
    _cmp(e1[0], e0[0], tol, "eager: the whole flat gradient, switch 1 against 0")
    _cmp(g1[1], g0[1], tol, "replayed: P0's flat gradient, switch 1 against 0")
    _cmp(g1[0], g0[0], tol, "replayed: the whole flat gradient, switch 1 against 0")
    scale = e1[0].abs().max().item()
    worst = (g1[0].double() - e1[0].double()).abs().max().item()
    print(f"{name}: replay against eager {worst:.3e} of {scale:.3e}")
    assert worst <= (2e-4 if f32 else BF16_TOL) * scale, (worst, scale)          # relative to the largest entry: the gradients are far below 1
    cos = torch.nn.functional.cosine_similarity(g1[0].double().flatten(), e1[0].double().flatten(), dim=0).item()
    assert cos >= (1 - 1e-8 if f32 else 1 - 3e-4), cos


def test_deterministic_runs_have_the_same_bits(hip, monkeypatch):
    for name in ("small_f32", "fused_bf16"):
        a = _trainer_grad(hip, name, 1, monkeypatch, steps=2, use_graph=True, deterministic=True)
        b = _trainer_grad(hip, name, 1, monkeypatch, steps=2, use_graph=True, deterministic=True)
        for (fa, _), (fb, _) in zip(a, b):
            assert fa.abs().max().item() > 0
            assert torch.equal(fa.view(torch.int16 if fa.element_size() == 2 else torch.int32),
                               fb.view(torch.int16 if fb.element_size() == 2 else torch.int32)), name


def test_replayed_steps_with_early_updates_track_the_eager_run(hip, monkeypatch):
    """Three optimiser steps, switch on: the replayed step of the split executor updates the last layers' matrices INSIDE the backward
    pass, before FanOutFn forms the value terms that read W_v -- the producers must have handed over the weights as they were
    (ops.SEG_SNAPSHOT_W).  Bound and exclusions of tests/test_train_gpu.py::test_replayed_and_deferred_steps_track_the_eager_run_
    parameter_for_parameter: 2e-4 of the largest parameter, key-projection biases (zero gradient up to rounding) left out."""
    from bist_amd import train
    args, model0, b = _setup(hip, "small_f32")
    monkeypatch.setenv(SWITCH, "1")
    res = {}
    for tag, kw in (("eager", dict(use_graph=False)), ("graph", dict(use_graph=True))):
        m = copy.deepcopy(model0)
        t = train.Trainer(m, args, 80, compute_dtype=torch.float32, warmup=20, factor=2.0, **kw)
        for _ in range(3):
            t.step(b)
        m.eval()
        torch.cuda.synchronize()
        res[tag] = {k: v.detach().clone() for k, v in m.named_parameters()}
    keys = [k for k in res["eager"] if not k.endswith("linears.1.bias")]
    scale = max(res["eager"][k].abs().max().item() for k in keys)
    worst, key = max(((res["eager"][k] - res["graph"][k]).abs().max().item(), k) for k in keys)
    print(f"three steps, replay against eager: {worst:.3e} at {key} (scale {scale:.3e})")
    assert worst <= 2e-4 * scale, (worst, key)


def test_model_gradients_match_reference_golden_with_the_switch_on(hip, monkeypatch, golden_dir):
    """the helper and bound of tests/test_train_gpu.py::test_model_gradients_match_reference_golden (1e-3 relative), switch on"""
    from bist_amd import _lib
    from bist_amd.data.batch import Batch
    from bist_amd.model.label_smoothing import LabelSmoothing
    from bist_amd.model.optimize import SimpleLossCompute
    M = hip
    monkeypatch.setenv(SWITCH, "1")
    g = np.load(os.path.join(golden_dir, "g3_model.npz"))
    meta = json.loads(str(g["both_cfg"]))
    cfg, dm = O.Cfg(**meta["cfg"]), meta["dims"]
    ob = O.det_batch(dm["B"], dm["T"], dm["S"], dm["C"], dm["Lq"], dm["Lh"], dm["Lc"], dm["Lt"], dm["V"])
    model = M.make_model(dm["V"], dm["V"], _args(cfg), ft_sizes=[dm["C"]])
    model.load_state_dict(O.det_state(cfg, dm["V"], dm["C"]), strict=False)
    model = model.cuda().eval()
    b = Batch(ob.query.cuda(), ob.his.cuda(), ob.fts.cuda(), ob.cap.cuda(), ob.trg.cuda(), ob.trg_y.cuda())
    lc = SimpleLossCompute(model.generator, model.ae_generator, LabelSmoothing(dm["V"], O.PAD_ID, 0.1), None, args=_args(cfg))
    terms, _ = lc.terms(model.forward(b), b)
    total = sum(terms.values())
    assert abs(total.item() - float(g["both_loss_total"])) < 1e-3 * abs(float(g["both_loss_total"]))
    _lib.lib.bist_launch_count_reset()
    total.backward()
    assert _lib.lib.bist_launch_count(_lib.K_GEMM_KSEG) >= 1
    sd = dict(model.named_parameters())
    worst = {}

    def cmp(name, ref):
        ref = torch.from_numpy(ref).double()
        got = sd[name].grad.double().cpu()
        worst[name] = ((got - ref).abs().max() / max(1e-4, ref.abs().max())).item()
    cmp("vid_encoder.W.weight", g["both_grad_vidW"])
    cmp("query_embed.0.lut.weight", g["both_grad_lut"])
    cmp("generator.pointer_gen_W.weight", g["both_grad_ptrW"])
    for ai in range(6):
        for j in range(4):
            if ai in (1, 2, 4, 5) and j == 1:
                continue
            cmp(f"mutlimodal_decoder.v_layers.0.attn.{ai}.linears.{j}.weight", g[f"both_grad_v0_attn{ai}_lin{j}_w"])
            cmp(f"mutlimodal_decoder.v_layers.0.attn.{ai}.linears.{j}.bias", g[f"both_grad_v0_attn{ai}_lin{j}_b"])
    for si in range(8):
        cmp(f"mutlimodal_decoder.v_layers.0.sublayer.{si}.norm.a_2", g[f"both_grad_v0_sub{si}_a"])
    bad = {k: v for k, v in worst.items() if not v <= 1e-3}
    assert not bad, f"relative gradient error > 1e-3: {bad}"


def test_trainerless_backward_passes_pin_nothing(hip, monkeypatch):
    """a training loop without bist_amd.train.Trainer never clears ops.WGRAD_KEEP: the segment operands must not be parked there (the
    allocator's record_stream covers them), whatever the number of passes"""
    from bist_amd import ops
    before = len(ops.WGRAD_KEEP)
    for _ in range(3):
        _, _, c1 = _autograd_grads(hip, "fused_bf16", 1, monkeypatch)
        assert c1[0] == 2
    assert len(ops.WGRAD_KEEP) == before


def test_a_rewrapped_placeholder_raises(hip, monkeypatch):
    """a producer that left its term in the sink returns an uninitialised zero-stride placeholder carrying a marker; a view between the
    alias and its consumer re-wraps the gradient and drops the marker: FanOutFn must refuse to sum it"""
    from bist_amd import functional as Fn
    monkeypatch.setenv(SWITCH, "1")
    B, T, S, d = 2, 4, 8, 128
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, T, S, d, generator=g).cuda().requires_grad_(True)
    w = (torch.randn(d, d, generator=g) * d ** -0.5).cuda().requires_grad_(True)

    def run(wrap):
        fan = Fn.Fan(x, 2)
        a, b_ = fan.take(), fan.take()
        if wrap:
            sink = a._bist_sink
            a = a.view(B, T, S, d)              # a view node: the tag is carried over by hand, the placeholder cannot be
            a._bist_sink = sink
        y = Fn.linear(a, w, None, leaf=True, out_shape=(B, T, S, d))
        (y.sum() + b_.sum()).backward()
        torch.cuda.synchronize()
    x.grad = None
    run(False)
    want = (torch.ones(B * T * S, d, device="cuda") @ w.detach()).view(B, T, S, d) + 1.0
    _cmp(x.grad, want, F32_TOL, "one value segment plus a gradient that arrived as a tensor")
    with pytest.raises(RuntimeError, match="placeholder"):
        run(True)
