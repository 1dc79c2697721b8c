"""Long-K products on at most 64 tiles of 64x64 take the ring kernel on 32x32 tiles (gemm_t32_ring_kernel: four times the
workgroups).  Every wave still walks the whole K range in tile order with the same MFMAs, so each output element sees the same
sequence of accumulations as in the 64x64 ring kernel: the automatic path must be BIT-identical to the same descriptor with the
hint BIST_GEMM_RING64, for every layout, dtype, epilogue, ragged tile and K tail -- and both agree with float64 to the tolerances
of tests/test_ops_gpu.py (F32_TOL / BF16_TOL there; repeated here because test modules do not import each other)."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

F32_TOL = 2e-5
BF16_TOL = 1.2e-2
RING64 = 8           # BIST_GEMM_RING64 (include/bist_hip.h)

SHAPES = [(320, 512, 2048), (320, 512, 1536), (37, 72, 1024), (100, 136, 1000), (33, 64, 776), (64, 512, 4096)]
DTYPES = [(torch.float32, F32_TOL), (torch.bfloat16, BF16_TOL)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from bist_amd import _lib, ops as o
    assert _lib.lib.bist_device_ok() == 1, _lib.lib.bist_last_error()
    assert o.GEMM_RING64 == RING64
    return o


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _takes(lay, M, N, dtype):
    """a row-contiguous operand is staged in 16-byte pieces along its rows: the row count must be whole pieces (make_plan)"""
    piece = 16 // torch.empty((), dtype=dtype).element_size()
    return (lay[0] == "N" or M % piece == 0) and (lay == "NT" or N % piece == 0)


CASES = [(dt, tol, lay, s) for dt, tol in DTYPES for lay in ("NT", "NN", "TT") for s in SHAPES if _takes(lay, s[0], s[1], dt)]


def _operands(M, N, K, lay, dtype, lead=()):
    a, b = _rand(*lead, M, K, seed=M + K), _rand(*lead, N, K, seed=N + K + 1, scale=K ** -0.5)
    aq, bq = a.to(dtype), b.to(dtype)
    A, ars, aks = (aq, K, 1) if lay[0] == "N" else (aq.transpose(-1, -2).contiguous(), 1, M)
    B, brs, bks = (bq, K, 1) if lay == "NT" else (bq.transpose(-1, -2).contiguous(), 1, N)
    return aq.double(), bq.double(), A.cuda(), B.cuda(), dict(a_rs=ars, a_ks=aks, b_rs=brs, b_ks=bks)


def _run(ops, A, B, out, hint, **kw):
    from bist_amd import _lib
    out.fill_(7.0)
    g = ops.gemm_desc(A, B, out, **kw)
    g.hint = hint
    assert _lib.lib.bist_gemm_is_fast(ctypes.byref(g)) >= 1          # an LDS-DMA kernel (2: K = 4096 in f32 is cut along K)
    _lib.check(_lib.lib.bist_gemm(ctypes.byref(g), torch.cuda.current_stream().cuda_stream), "bist_gemm")
    return out


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _both(ops, A, B, shape, out_dtype, what, **kw):
    """the product with the automatic choice and with the 64x64 ring forced: the same bits; returns the automatic result"""
    auto = _run(ops, A, B, torch.empty(*shape, device="cuda", dtype=out_dtype), 0, **kw).clone()
    old = _run(ops, A, B, torch.empty(*shape, device="cuda", dtype=out_dtype), RING64, **kw)
    assert torch.equal(_bits(auto), _bits(old)), what
    return auto


def _cmp(got, ref, tol, what):
    got = got.detach().float().cpu().double()
    err = (got - ref).abs().max().item()
    scale = max(1.0, ref.abs().max().item())
    assert math.isfinite(err) and err <= tol * scale, f"{what}: max err {err:.3e} (scale {scale:.3e}, tol {tol})"


@pytest.mark.parametrize("dtype,tol,lay,shape", CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_fine_tile_bits_equal_the_64_tile_ring(ops, monkeypatch, dtype, tol, lay, shape):
    M, N, K = shape
    a6, b6, A, B, st = _operands(M, N, K, lay, dtype)
    bias, res = _rand(N, seed=3).to(dtype), _rand(M, N, seed=4).to(dtype)
    inner, outer = 8, 16                                                    # row m adds residual row (m / 16) * 8 + m % 8
    rmap = _rand((M + outer - 1) // outer * inner, N, seed=5).to(dtype)
    kw = dict(M=M, N=N, K=K, ldc=N, **st)
    ref = a6 @ b6.t()
    check64 = shape in SHAPES[:4]                                           # against float64: the first four shapes

    out = _both(ops, A, B, (M, N), dtype, "bias", bias=bias.cuda(), **kw)
    if check64:
        _cmp(out, ref + bias.double(), tol, "bias")

    monkeypatch.setattr(ops, "DROP_CTR", torch.tensor([5], dtype=torch.int64, device="cuda"))
    p = 0.25
    out = _both(ops, A, B, (M, N), dtype, "bias + ReLU + dropout", bias=bias.cuda(), act=ops.ACT_RELU, drop_p=p, drop_seed=77, **kw)
    monkeypatch.setattr(ops, "DROP_CTR", None)
    if check64:
        o, want = out.float().cpu().double(), (ref + bias.double()).clamp_min(0)
        kept = o != 0
        _cmp(torch.where(kept, o * (1 - p), torch.zeros(())), torch.where(kept, want, torch.zeros(())), tol, "dropout")
        if M * N >= 10000:
            assert abs(kept.double().mean().item() - (1 - p) * (want > 0).double().mean().item()) < 2e-2

    out = _both(ops, A, B, (M, N), dtype, "residual with alpha", bias=bias.cuda(), residual=res.cuda(), ldr=N, alpha=0.5, **kw)
    if check64:
        _cmp(out, 0.5 * ref + bias.double() + res.double(), tol, "residual with alpha")

    out = _both(ops, A, B, (M, N), dtype, "row-mapped residual", residual=rmap.cuda(), ldr=N, res_map=(outer, inner), **kw)
    if check64:
        rows = torch.arange(M)
        _cmp(out, ref + rmap.double()[(rows // outer) * inner + rows % inner], tol, "row-mapped residual")

    if dtype == torch.bfloat16:
        out = _both(ops, A, B, (M, N), torch.float32, "f32 output from bf16 operands", **kw)
        if check64:
            _cmp(out, ref, 2e-3, "f32 output from bf16 operands")


@pytest.mark.parametrize("dtype,tol", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("lay", ["NT", "NN"])
def test_fine_tile_batched_with_strides(ops, dtype, tol, lay):
    M, N, K, nb = 100, 136, 1000, 2
    a6, b6, A, B, st = _operands(M, N, K, lay, dtype, lead=(nb,))
    bias = _rand(N, seed=3).to(dtype)
    kw = dict(M=M, N=N, K=K, ldc=N, batch=(nb, 1), a_bs=(M * K, 0), b_bs=(N * K, 0), c_bs=(M * N, 0), bias=bias.cuda(), **st)
    out = _both(ops, A, B, (nb, M, N), dtype, "batched", **kw)
    _cmp(out, a6 @ b6.transpose(-1, -2) + bias.double(), tol, "batched")


@pytest.mark.parametrize("M,N,K", [(320, 512, 512), (576, 512, 1024)])
def test_shapes_just_outside_the_fine_tile_envelope(ops, M, N, K):
    """eight K tiles (the all-in-flight kernel) and 72 tiles of 64x64 (the 64x64 ring): the hint changes nothing"""
    dtype, tol = torch.bfloat16, BF16_TOL
    a6, b6, A, B, st = _operands(M, N, K, "NT", dtype)
    bias = _rand(N, seed=3).to(dtype)
    out = _both(ops, A, B, (M, N), dtype, "outside the envelope", M=M, N=N, K=K, ldc=N, bias=bias.cuda(), **st)
    _cmp(out, a6 @ b6.t() + bias.double(), tol, "outside the envelope")


@pytest.mark.parametrize("lay", ["NT", "NN"])
def test_fine_tile_repeats_on_cold_operands(ops, lay):
    """The 32x32 ring orders its LDS-DMA stagings against the fragment reads by counted vmcnt waits and barriers only; a misplaced
    wait shows as a rare wrong tile that comes and goes with the memory system's timing.  Screen: the feed-forward product 24 times,
    each time after 320 MB of other traffic has evicted the operands from every cache (the weights of a training step are cold in the
    same way) -- every result bit-identical to the 64x64 ring's."""
    M, N, K = 320, 512, 2048
    dtype = torch.bfloat16
    _, _, A, B, st = _operands(M, N, K, lay, dtype)
    kw = dict(M=M, N=N, K=K, ldc=N, **st)
    want = _run(ops, A, B, torch.empty(M, N, device="cuda", dtype=dtype), RING64, **kw).clone()
    flush = torch.empty(320 << 20, device="cuda", dtype=torch.uint8)
    out = torch.empty(M, N, device="cuda", dtype=dtype)
    for rep in range(24):
        flush.fill_(rep)
        assert torch.equal(_bits(_run(ops, A, B, out, 0, **kw)), _bits(want)), f"run {rep} differs from the 64x64 ring"
