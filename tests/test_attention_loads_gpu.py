"""The three attention cores whose operand loads are issued ahead of the first wait (stage 2 on the matrix cores, the
small attention forward, the small attention backward on the matrix cores): every edge of the clamped rows / columns
and of the 32 / 64 / 128-row images against float64 on the bf16-rounded inputs.

Bounds are those of the existing tests of the same ops (repeated here because test modules do not import each other):
stage 2: 1.5e-2 forward, 2.5e-2 dq2f / dY (test_stage2_bf16_matrix_core_path); small attention: 1.5e-2 output, 3e-2
dQ / dKV (test_mha_core_backward_bf16_matrix_core_path), both relative to max(1e-3, max |ref|); small attention forward
alone: BF16_TOL / F32_TOL of tests/test_ops_gpu.py, relative to max(1, max |ref|), probabilities 1e-2 / 1e-5."""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

F32_TOL = 2e-5
BF16_TOL = 1.2e-2
BF = torch.bfloat16


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from bist_amd import functional as Fn, ops
    return Fn, ops


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def _close(got, ref, what, tol):
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs().max().item()
    sc = max(1e-3, ref.abs().max().item())
    assert math.isfinite(err) and err <= tol * sc, f"{what}: err {err:.3e} scale {sc:.3e}"


def _cmp(got, ref, tol, what):
    got = got.detach().float().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs().max().item()
    scale = max(1.0, ref.abs().max().item())
    assert math.isfinite(err) and err <= tol * scale, f"{what}: max err {err:.3e} (scale {scale:.3e}, tol {tol})"


# ---------------------------------------------------------------------------------------------------------------------
# stage 2
# ---------------------------------------------------------------------------------------------------------------------
ST2_G = [1, 2, 31, 32, 33, 48, 49, 55, 56, 57, 63, 64, 65, 127, 128]
ST2_SHAPES = [(1, 1, 1, 128), (2, 3, 5, 256), (3, 20, 8, 512)]


def _st2_mask(kind, B, G):
    if kind == "none":
        return None
    gm = torch.ones(B, 1, G, dtype=torch.bool)
    if kind == "tail":
        gm[0, 0, G // 3:] = False
    else:                                    # one fully masked clip: uniform probabilities, no NaN
        gm[B - 1] = False
    return gm


def _st2_inputs(B, G, Lq, h, d):
    q2f = _rand(B, Lq, h, d, seed=70, scale=d ** -0.5).to(BF).double()
    y = _rand(B, G, Lq, d, seed=71).to(BF).double()
    go = _rand(B, Lq, h, d, seed=72).to(BF).double()
    return q2f, y, go


def _st2_ref(q2f, y, go, gm):
    B, G = y.shape[:2]
    qr, yr = q2f.clone().requires_grad_(True), y.clone().requires_grad_(True)
    sc = torch.einsum("bihe,bgie->bihg", qr, yr)
    if gm is not None:
        sc = sc.masked_fill(gm.view(B, 1, 1, G) == 0, -1e9)
    p = torch.softmax(sc, -1)
    ref = torch.einsum("bihg,bgie->bihe", p, yr)
    (ref * go).sum().backward()
    return ref.detach(), qr.grad, yr.grad, p.detach()


def _st2_run(Fn, q2f, y, go, gm, h, drop=None):
    qd = q2f.to(BF).cuda().requires_grad_(True)
    yd = y.to(BF).cuda().requires_grad_(True)
    out, rs = Fn.st_stage2(qd, yd, None if gm is None else gm.cuda(), h=h, drop=drop)
    (out.double() * go.cuda()).sum().backward()
    return out.detach(), qd.grad, yd.grad, rs


@pytest.mark.parametrize("B,Lq,h,d", ST2_SHAPES)
@pytest.mark.parametrize("G", ST2_G)
def test_stage2_image_edges(env, G, B, Lq, h, d):
    Fn, ops = env
    q2f, y, go = _st2_inputs(B, G, Lq, h, d)
    for kind in ("none", "tail", "clip"):
        gm = _st2_mask(kind, B, G)
        ref, dq, dy, p = _st2_ref(q2f, y, go, gm)
        out, gq, gy, _ = _st2_run(Fn, q2f, y, go, gm, h)
        _close(out, ref, f"st2 fwd ({kind})", 1.5e-2)
        _close(gq, dq, f"st2 dq2f ({kind})", 2.5e-2)
        _close(gy, dy, f"st2 dY ({kind})", 2.5e-2)
        if kind == "clip":
            assert (p[B - 1] - 1.0 / G).abs().max().item() < 1e-12          # (the reference itself: uniform)
            _close(out[B - 1], y[B - 1].mean(0).unsqueeze(1).expand(Lq, h, d), "st2 fwd of the masked clip = mean of Y", 1.5e-2)


@pytest.mark.parametrize("G", ST2_G)
def test_stage2_nan_in_next_clip(env, G):
    """The last clip's Y is NaN: a read of a row >= G of clip 1 (which is the next clip's memory) would show as NaN x 0."""
    Fn, ops = env
    B, Lq, h, d = 3, 20, 8, 512
    q2f, y, go = _st2_inputs(B, G, Lq, h, d)
    gm = _st2_mask("tail", B, G)
    ref, dq, dy, _ = _st2_ref(q2f[:2], y[:2], go[:2], gm[:2])
    yn = y.clone()
    yn[2] = float("nan")
    out, gq, gy, _ = _st2_run(Fn, q2f, yn, go, gm, h)
    for t in (out[:2], gq[:2], gy[:2]):
        assert torch.isfinite(t.float()).all()
    _close(out[:2], ref, "st2 fwd", 1.5e-2)
    _close(gq[:2], dq, "st2 dq2f", 2.5e-2)
    _close(gy[:2], dy, "st2 dY", 2.5e-2)


@pytest.mark.parametrize("G", ST2_G)
def test_stage2_dropout_rowsum(env, G):
    """Probability dropout: column 0 of Y is 1, so PY[..., 0] is the sum of the dropped probabilities that the kernel also
    reports as rowsum (bound: the forward's, the sum runs over bf16 probabilities); two launches are bit-equal."""
    Fn, ops = env
    B, Lq, h, d = 2, 3, 5, 256
    q2f, y, go = _st2_inputs(B, G, Lq, h, d)
    y[..., 0] = 1.0
    gm = _st2_mask("tail", B, G)
    a = _st2_run(Fn, q2f, y, go, gm, h, drop=(0.1, 1234))
    b = _st2_run(Fn, q2f, y, go, gm, h, drop=(0.1, 1234))
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    out, _, _, rs = a
    assert rs is not None and rs.shape == (B, Lq, h)
    _close(out[..., 0], rs.double().cpu(), "st2 rowsum", 1.5e-2)
    assert rs.max().item() <= 1.0 / 0.9 + 1e-5                   # kept probabilities are scaled by 1 / (1 - p) and sum to at most 1


@pytest.mark.parametrize("B,Lq,h,d", ST2_SHAPES)
@pytest.mark.parametrize("G", [1, 2, 31, 32, 33])
def test_stage2_backward_image_forms_bit_equal(env, G, B, Lq, h, d):
    """BIST_ST2_BWD_FULL=1 keeps the backward's 64-row images at G <= 32: the same bits as the 32-row form."""
    Fn, ops = env
    q2f, y, go = _st2_inputs(B, G, Lq, h, d)
    gm = _st2_mask("tail", B, G)
    old = os.environ.get("BIST_ST2_BWD_FULL")
    try:
        for drop in (None, (0.1, 99)):           # (under dropout the probabilities carry a factor that is not 1: rounding points show)
            os.environ["BIST_ST2_BWD_FULL"] = "1"
            full = _st2_run(Fn, q2f, y, go, gm, h, drop=drop)
            os.environ["BIST_ST2_BWD_FULL"] = "0"
            half = _st2_run(Fn, q2f, y, go, gm, h, drop=drop)
            for u, v in zip(full[:3], half[:3]):
                assert torch.equal(u.view(torch.int16), v.view(torch.int16))
    finally:
        if old is None:
            os.environ.pop("BIST_ST2_BWD_FULL", None)
        else:
            os.environ["BIST_ST2_BWD_FULL"] = old


# ---------------------------------------------------------------------------------------------------------------------
# small attention
# ---------------------------------------------------------------------------------------------------------------------
def _ref_attn(q, k, v, mask, h):
    N, Lq, d = q.shape
    Lk, dk = k.shape[1], d // h
    q4, k4, v4 = (t.view(N, -1, h, dk).transpose(1, 2) for t in (q, k, v))
    sc = q4 @ k4.transpose(-1, -2) / math.sqrt(dk)
    if mask is not None:
        sc = sc.masked_fill(mask.unsqueeze(1) == 0, -1e9)
    p = torch.softmax(sc, -1)
    return (p @ v4).transpose(1, 2).reshape(N, Lq, d), p


def _attn_mask(kind, N, Lq, Lk):
    if kind == "key":
        m = torch.ones(N, 1, Lk, dtype=torch.bool)
        m[0, 0, Lk // 2:] = False
        m[N - 1] = False                       # whole last clip: uniform 1 / Lk
        return m
    if kind == "causal":
        return torch.tril(torch.ones(1, Lq, Lk, dtype=torch.bool)).expand(N, Lq, Lk).clone()
    return None


MHA_SHAPES = [(1, 1, 1, 1, 64), (3, 20, 20, 8, 64), (2, 20, 25, 8, 64), (2, 20, 60, 8, 64), (2, 20, 64, 8, 64), (2, 6, 130, 1, 64),
              (4, 20, 25, 1, 512), (2, 5, 7, 4, 16), (2, 4, 11, 2, 32)]


@pytest.mark.parametrize("dtype,tol,ptol", [(torch.float32, F32_TOL, 1e-5), (BF, BF16_TOL, 1e-2)])
@pytest.mark.parametrize("N,Lq,Lk,h,dk", MHA_SHAPES)
def test_mha_core_fetch_ahead(env, N, Lq, Lk, h, dk, dtype, tol, ptol):
    """q / k / v are column slices of one packed buffer (rows of 3 d elements)."""
    Fn, ops = env
    d, L = h * dk, max(Lq, Lk)
    buf = _rand(N, L, 3 * d, seed=16)
    buf[..., :d] *= (64.0 / dk) ** 0.5
    buf = buf.to(dtype)
    bq = buf.double()
    qr, kr, vr = bq[:, :Lq, :d], bq[:, :Lk, d:2 * d], bq[:, :Lk, 2 * d:]
    dev = buf.cuda()
    q, k, v = dev[:, :Lq, :d], dev[:, :Lk, d:2 * d], dev[:, :Lk, 2 * d:]
    from bist_amd import _lib
    ahead0 = _lib.lib.bist_launch_count(_lib.K_MHA_FWD_DK64)
    for kind, want_p in (("key", False), ("causal", False), ("none", False), ("key", True)):
        mask = _attn_mask(kind, N, Lq, Lk)
        ref, pref = _ref_attn(qr, kr, vr, mask, h)
        out, p = ops.mha_core(q, k, v, None if mask is None else mask.cuda(), h, want_p=want_p)
        _cmp(out, ref, tol, f"mha_core out ({kind})")
        if want_p:
            _cmp(p, pref, ptol, "mha_core p_attn")
            assert torch.allclose(p[N - 1].cpu(), torch.full_like(p[N - 1].cpu(), 1.0 / Lk), atol=1e-6)
    mask = _attn_mask("key", N, Lq, Lk).cuda()
    a = ops.mha_core(q, k, v, mask, h, want_p=True, drop=(0.1, 77))
    b = ops.mha_core(q, k, v, mask, h, want_p=True, drop=(0.1, 77))
    assert torch.equal(a[0].view(torch.uint8), b[0].view(torch.uint8)) and torch.equal(a[1], b[1])
    _cmp(a[1], _ref_attn(qr, kr, vr, mask.cpu(), h)[1], ptol, "mha_core p_attn under dropout (the probabilities before it)")
    # which kernel ran: the fetch-ahead form for bf16, dk = 64, Lk <= 64 (all six launches above), the generic one otherwise
    ahead = _lib.lib.bist_launch_count(_lib.K_MHA_FWD_DK64) - ahead0
    assert ahead == (6 if (dtype == BF and dk == 64 and Lk <= 64) else 0), ahead


@pytest.mark.parametrize("dk", [64, 192])
@pytest.mark.parametrize("h", [1, 8])
@pytest.mark.parametrize("Lq", [1, 20, 32])
@pytest.mark.parametrize("Lk", [1, 7, 8, 9, 20, 25, 60, 63, 64])
def test_mha_backward_mask_edges(env, Lk, Lq, h, dk):
    """Through Fn.mha_packed, with a gradient arriving through the probabilities as well."""
    Fn, ops = env
    N, d = 2, h * dk
    q = _rand(N, Lq, d, seed=80, scale=(64.0 / dk) ** 0.5).to(BF).double()
    kv = _rand(N, Lk, 2 * d, seed=81).to(BF).double()
    wo, wp = _rand(N, Lq, d, seed=82).to(BF).double(), _rand(N, h, Lq, Lk, seed=83)
    for kind in ("key", "causal", "none"):
        mask = _attn_mask(kind, N, Lq, Lk)
        qr, kvr = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
        ro, rp = _ref_attn(qr, kvr[..., :d], kvr[..., d:], mask, h)
        ((ro * wo).sum() + (rp * wp).sum()).backward()
        qd, kvd = q.to(BF).cuda().requires_grad_(True), kv.to(BF).cuda().requires_grad_(True)
        o, p = Fn.mha_packed(qd, kvd, None, "q_kv", None if mask is None else mask.cuda(), h, True)
        ((o.double() * wo.cuda()).sum() + (p.double() * wp.cuda()).sum()).backward()
        _close(o, ro.detach(), f"mha bf16 out ({kind})", 1.5e-2)
        _close(qd.grad, qr.grad, f"mha bf16 dQ ({kind})", 3e-2)
        _close(kvd.grad, kvr.grad, f"mha bf16 dKV ({kind})", 3e-2)


# ---------------------------------------------------------------------------------------------------------------------
# screen of the waits: operands from HBM (a 512 MB fill between launches), every repeat bit-equal to the first
# ---------------------------------------------------------------------------------------------------------------------
def _bits(ts):
    return [t.detach().clone().view(torch.int16) for t in ts]


def _screen(run, n=24):
    fill = torch.empty(512 * 1024 * 1024, dtype=torch.uint8, device="cuda")
    first = None
    for r in range(n):
        fill.fill_(r)
        got = _bits(run())
        if first is None:
            first = got
        else:
            for u, v in zip(first, got):
                assert torch.equal(u, v), f"repeat {r} differs from the first launch"


@pytest.mark.parametrize("G", [49, 32])
def test_stage2_repeats_bit_equal(env, G):
    Fn, ops = env
    B, Lq, h, d = 16, 20, 8, 512
    q2f, y, go = _st2_inputs(B, G, Lq, h, d)
    gm = _st2_mask("tail", B, G)
    qd, yd, gd, md = q2f.to(BF).cuda().requires_grad_(True), y.to(BF).cuda().requires_grad_(True), go.to(BF).cuda(), gm.cuda()

    def run():
        qd.grad = yd.grad = None
        out, _ = Fn.st_stage2(qd, yd, md, h=h)
        out.backward(gd)
        return out, qd.grad, yd.grad
    _screen(run)


def test_mha_repeats_bit_equal(env):
    Fn, ops = env
    N, Lq, Lk, h, dk = 16, 20, 20, 8, 64
    d = h * dk
    qd = _rand(N, Lq, d, seed=80).to(BF).cuda().requires_grad_(True)
    kvd = _rand(N, Lk, 2 * d, seed=81).to(BF).cuda().requires_grad_(True)
    gd = _rand(N, Lq, d, seed=82).to(BF).cuda()
    md = _attn_mask("key", N, Lq, Lk).cuda()

    def run():
        qd.grad = kvd.grad = None
        o, _ = Fn.mha_packed(qd, kvd, None, "q_kv", md, h, False)
        o.backward(gd)
        return o, qd.grad, kvd.grad
    _screen(run)
