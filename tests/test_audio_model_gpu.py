"""The audio modality against the REFERENCE run with its audio stack on (tests/golden/g9_audio*.npz, written by
tests/golden/make_golden_audio.py; the CPU oracle does not model audio): VGGish-like features through the input stage, the audio
reasoning layers, the five-part fusion (or the seventh decoder attention), the audio auto-encoder loss, forward and backward.

fp32, every small case: each stored tensor and the log-probs within 1e-3 of the reference with identical argmax
(tests/test_model_gpu.py:21, 82-84), loss terms within 1e-3 max(1, |ref|) (test_model_gpu.py:93), gradients within 1e-3 of the tensor's
largest entry (tests/test_train_gpu.py:448, 460).
bf16, wide case (d_model = 512; weights and inputs bf16-representable on both sides, as tests/test_production_gpu.py:44-48 prepares
them): the sampled values of the digests within 6e-2 absolute (test_production_gpu.py:80), >= 90 % identical argmax (:82-83), loss terms
within 2 % (:139), gradient samples with cosine >= 0.995 and max error <= 8 % of the tensor's largest entry (:147).
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audio_util as AU                                   # noqa: E402

from oracle import bist_oracle as O                       # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    import bist_amd.model as M
    from bist_amd.data.batch import Batch
    return M, Batch


@pytest.fixture(scope="module")
def goldens(golden_dir):
    return {f: np.load(os.path.join(golden_dir, f + ".npz")) for f in ("g9_audio", "g9_audio_none", "g9_audio_wide")}


def _case(hip, g, tag, dtype=torch.float32, args_extra=None):
    return AU.model_case(g, tag, dtype, args_extra)


def _err(a, b):
    return (a.detach().float().cpu().double() - torch.as_tensor(b).double()).abs().max().item()


def _terms(model, b, args, V):
    from bist_amd.model.label_smoothing import LabelSmoothing
    from bist_amd.model.optimize import SimpleLossCompute
    return SimpleLossCompute(model.generator, model.ae_generator, LabelSmoothing(V, O.PAD_ID, 0.1), None, args=args)


@pytest.mark.parametrize("tag", ["dyn", "nocap", "zerosum", "long", "none"])
def test_small_cases_match_the_reference_fp32(hip, goldens, tag):
    g = goldens["g9_audio_none" if tag == "none" else "g9_audio"]
    model, b, meta, args = _case(hip, g, tag)
    dm = meta["dims"]
    assert np.array_equal(b.audio_mask.cpu().numpy(), g[f"{tag}_audio_mask"])          # device-side mask == dataset.py:87
    if tag == "zerosum":
        r = meta["dims"]["zero_sum_row"]
        assert not b.audio_mask[r[0], 0, r[1]] and (b.audio_fts[r[0], r[1]] != 0).any()
    lc = _terms(model, b, args, dm["V"])
    with torch.no_grad():
        ft = model.forward(b)
        terms, logp = lc.terms(ft, b)
    worst = {k[len(tag) + 4:]: _err(ft[k[len(tag) + 4:]], g[k]) for k in g.files if k.startswith(f"{tag}_ft_")}
    worst["logp"] = _err(logp, g[f"{tag}_logp"])
    print(tag, "forward errors", worst)
    bad = {k: v for k, v in worst.items() if not v <= 1e-3}
    assert not bad, f"beyond 1e-3 of the reference: {bad} (all: {worst})"
    assert torch.equal(logp.argmax(-1).cpu(), torch.from_numpy(g[f"{tag}_logp"]).argmax(-1))
    if tag == "dyn":
        assert {"encoded_audio", "audio_ft", "encoded_ft", "cap_ft", "temporal_ft", "spatial_ft", "decoded_text"} <= set(worst)
    want_terms = [k[len(tag) + 6:] for k in g.files if k.startswith(f"{tag}_loss_") and not k.endswith("_total")]
    assert sorted(terms) == sorted(want_terms)
    if meta["cfg"]["nb_cenc_blocks"] > 0:
        assert list(terms) == ["out", "cap_ae", "audio_ae", "temporal_ae", "spatial_ae"]          # optimize.py:55-82
    for name, val in terms.items():
        ref = float(g[f"{tag}_loss_{name}"])
        assert abs(val.item() - ref) <= 1e-3 * max(1.0, abs(ref)), (name, val.item(), ref)
    grads = [k for k in g.files if k.startswith(f"{tag}_grad_")]
    if not grads:
        return
    # backward through the training forms (eval(): dropout off, as in the capture)
    model.zero_grad(set_to_none=True)
    ft = model.forward(b)
    terms, _ = lc.terms(ft, b)
    total = sum(terms.values())
    assert abs(total.item() - float(g[f"{tag}_loss_total"])) < 1e-3 * abs(float(g[f"{tag}_loss_total"]))
    total.backward()
    torch.cuda.synchronize()
    sd = dict(model.named_parameters())
    worst = {}
    for k in grads:
        name = k[len(tag) + 6:]
        ref = torch.from_numpy(g[k]).double()
        got = sd[name].grad.double().cpu()
        worst[name] = ((got - ref).abs().max() / max(1e-4, ref.abs().max())).item()
    print(tag, "worst gradient errors", sorted(worst.items(), key=lambda e: -e[1])[:5])
    bad = {k: v for k, v in worst.items() if not v <= 1e-3}
    assert not bad, f"relative gradient error > 1e-3: {bad}"
    if tag == "dyn":
        assert any("a_layers.1.attn.1" in k for k in worst) and "vid_encoder.a_W.weight" in worst
        assert "mutlimodal_decoder.vc_combine_W.weight" in worst and AU.LUT in worst
    if tag == "none":
        assert sum(".attn.6." in k for k in worst) == 2 * 8           # the seventh attention of both decoder layers


def _samples(dg):
    """(values, their flat indices are implied by the digest form) the 128 sampled values of a digest."""
    return torch.from_numpy(np.asarray(dg[2:]))


def _sampled(t, k=64):
    x = t.detach().double().reshape(-1).cpu()
    idx = torch.linspace(0, x.numel() - 1, k).long()
    return torch.cat([x[:k], x[idx]])


@pytest.fixture(scope="module")
def wide(hip, goldens):
    g = goldens["g9_audio_wide"]
    model, b, meta, args = _case(hip, g, "wide", dtype=torch.bfloat16)
    return g, model, b, meta, args


def test_wide_bf16_training_path_matches_the_reference_digests(wide, monkeypatch):
    from bist_amd import _lib
    g, model, b, meta, args = wide
    dm = meta["dims"]
    calls = []
    real = _lib.lib.bist_switch_logits_fwd
    monkeypatch.setattr(_lib.lib, "bist_switch_logits_fwd", lambda parts, n, *a: calls.append(n) or real(parts, n, *a))
    model.zero_grad(set_to_none=True)
    lc = _terms(model, b, args, dm["V"])
    ft = model.forward(b)
    n_forward = list(calls)
    terms, logp = lc.terms(ft, b)
    total = sum(terms.values())
    total.backward()
    torch.cuda.synchronize()
    # the fusion logits of every block are ONE five-part launch in the training forward: a product per part is a failure
    assert n_forward.count(5) == meta["cfg"]["nb_blocks"], n_forward
    worst = {}
    for k in [k for k in g.files if k.startswith("wide_dg_")]:
        name = k[len("wide_dg_"):]
        t = logp if name == "logp" else ft[name]
        assert t.numel() >= 1
        worst[name] = (_sampled(t) - _samples(g[k])).abs().max().item()
    print("wide forward errors", worst)
    bad = {k: v for k, v in worst.items() if not v <= 6e-2}
    assert not bad, f"beyond the bf16 bound of the reference: {bad} (all: {worst})"
    for k in ("encoded_audio", "audio_ft", "encoded_ft", "cap_ft", "temporal_ft", "spatial_ft", "decoded_text", "logp"):
        assert k in worst, k
    agree = (logp.argmax(-1).cpu().numpy() == g["wide_argmax"]).mean()
    assert agree >= 0.9, agree
    assert list(terms) == ["out", "cap_ae", "audio_ae", "temporal_ae", "spatial_ae"]
    for name, val in terms.items():
        ref = float(g[f"wide_loss_{name}"])
        assert abs(val.item() - ref) <= 2e-2 * max(1.0, abs(ref)), (name, val.item(), ref)
    sd = dict(model.named_parameters())
    audio = [k for k in sd if any(s in k for s in ("vid_encoder.a_W", "vid_encoder.a_in_norm", ".a_layers.", ".a_out_norm."))
             and (k.endswith(".weight") or k.endswith(".a_2"))]
    keys = audio + ["vid_encoder.W.weight", "vid_encoder.in_norm.a_2", "query_embed.0.lut.weight", "generator.pointer_gen_W.weight",
                    "mutlimodal_decoder.vc_combine_W.weight", "mutlimodal_decoder.layers.1.attn.0.linears.0.weight",
                    "mutlimodal_decoder.c_layers.0.attn.1.linears.2.weight"]
    assert len(audio) == 2 + 2 * (8 + 2 + 3) + 1
    bad = {}
    for k in keys:
        ref = _samples(g[f"wide_gdg_{k}"])
        got = _sampled(sd[k].grad)
        cos = torch.nn.functional.cosine_similarity(got, ref, dim=0).item()
        rel = ((got - ref).abs().max() / max(1e-8, float(g[f"wide_gmax_{k}"]))).item()
        if not (cos >= 0.995 and rel <= 8e-2):
            bad[k] = (cos, rel)
    assert not bad, f"gradient (cosine, max relative error) out of the bf16 bound: {bad}"


def test_wide_bf16_inference_path_matches_the_reference_digests(wide):
    g, model, b, meta, args = wide
    with torch.no_grad():
        ft = model.forward(b)
        logp = model.generator(ft, b, args)
    worst = {}
    for k in [k for k in g.files if k.startswith("wide_dg_")]:
        name = k[len("wide_dg_"):]
        worst[name] = (_sampled(logp if name == "logp" else ft[name]) - _samples(g[k])).abs().max().item()
    print("wide inference errors", worst)
    bad = {k: v for k, v in worst.items() if not v <= 6e-2}
    assert not bad, f"beyond the bf16 bound of the reference: {bad} (all: {worst})"
    assert (logp.argmax(-1).cpu().numpy() == g["wide_argmax"]).mean() >= 0.9


def test_audio_input_stage_is_the_same_through_the_layernorm_epilogue(wide, monkeypatch):
    """Inference runs encoded_audio = a_in_norm(ReLU(a_W audio)) through the product's LayerNorm epilogue where it covers the shape
    (bf16, whole 256-row tiles: B * Ta = 8 * 32 here; Da = 128 is the epilogue kernel's smallest K); training keeps the product and the
    LayerNorm apart for the backward.  The test asserts that the epilogue launch IS taken (bist_gemm_ln_ok on the descriptor ops.linear
    builds, the 256-tile kernel, and no LayerNorm launch), then compares it with the separate form.  The two forms differ by one bf16
    rounding of the activation ahead of the LayerNorm and one of each output: per rounding 2^-9 relative; the LayerNorm is invariant
    to the activation's scale, so an activation error of 2^-9 |act| moves an output by about 2^-9 |y| through the deviation, the mean
    and the spread (three addends), plus the two output roundings -- 5 x 2^-9, bounded here by 2^-6 max(1, |y|max)."""
    import ctypes as C
    import types
    from bist_amd import _lib, functional as Fn, ops
    g, model, b, meta, args = wide
    enc = model.vid_encoder
    monkeypatch.setattr(enc, "v_N", 0)                    # the audio stage alone
    B, Ta, Da = 8, 32, 128
    au = torch.from_numpy(AU.audio_input(B, Ta, Da, 977, zero_tail=((1, 3), (5, 10)))).cuda().to(torch.bfloat16)
    ab = types.SimpleNamespace(fts=None, audio_fts=au)
    n = enc.a_in_norm
    x2, out = au.reshape(B * Ta, Da), torch.empty(B * Ta, 512, device="cuda", dtype=torch.bfloat16)
    gd = ops.gemm_desc(x2, enc.a_W.weight, out, M=B * Ta, N=512, K=Da, a_rs=Da, b_rs=enc.a_W.weight.stride(0), ldc=512, bias=enc.a_W.bias,
                       act=Fn.ACT_RELU)
    gd.ln_gain, gd.ln_offset, gd.ln_eps, gd.ln_mode = n.a_2.data_ptr(), n.b_2.data_ptr(), n.eps, 1
    assert _lib.lib.bist_gemm_ln_ok(C.byref(gd)) == 1 and _lib.lib.bist_gemm_is_fast(C.byref(gd)) == 4
    ln_calls = []
    real_ln = ops.layernorm
    monkeypatch.setattr(ops, "layernorm", lambda *a, **k: ln_calls.append(1) or real_ln(*a, **k))
    outs, launches = {}, {}
    for form, epi in (("epilogue", True), ("separate", False)):
        monkeypatch.setattr(ops, "LN_EPILOGUE", epi)
        del ln_calls[:]
        with torch.no_grad():
            outs[form] = enc(ab, {})["encoded_audio"].float()
        launches[form] = len(ln_calls)
    assert launches == {"epilogue": 0, "separate": 1}, launches          # one launch against product + LayerNorm
    outs["training"] = enc(ab, {})["encoded_audio"].detach().float()
    torch.cuda.synchronize()
    ref = torch.relu(au.float() @ enc.a_W.weight.float().t() + enc.a_W.bias.float())
    ref = n.a_2.float() * (ref - ref.mean(-1, keepdim=True)) / (ref.std(-1, keepdim=True) + n.eps) + n.b_2.float()
    bound = 2.0 ** -6 * max(1.0, ref.abs().max().item())
    for form in ("epilogue", "separate", "training"):
        err = (outs[form] - ref.view(B, Ta, -1)).abs().max().item()
        print("encoded_audio", form, "vs f32 arithmetic:", err, "bound", bound)
        assert tuple(outs[form].shape) == (B, Ta, 512) and err <= bound, (form, err, bound)
    err = (outs["epilogue"] - outs["separate"]).abs().max().item()
    print("encoded_audio epilogue vs separate:", err)
    assert err <= bound
    assert (outs["separate"] - outs["training"]).abs().max().item() <= bound


def test_fusion_fallback_is_one_product_per_part_and_agrees(hip, goldens, monkeypatch):
    """BIST_FUSE_ONE_LAUNCH=0 (autograd.FUSE_ONE_LAUNCH): the five products per block the one-launch form replaces give the reference's
    result too -- the comparison DESIGN.md section 18 times."""
    from bist_amd import autograd as ag
    g = goldens["g9_audio"]
    model, b, meta, args = _case(hip, g, "dyn")
    monkeypatch.setattr(ag, "FUSE_ONE_LAUNCH", False)
    ft = model.forward(b)
    assert _err(ft["encoded_ft"], g["dyn_ft_encoded_ft"]) <= 1e-3
