"""bist_gemm_kseg: C = alpha * sum_s A_s . B_s^T (+ residual) as ONE launch of the 128x128-tile kernel, the accumulators kept in
registers across the segments.  Both layout groups the video tensor's gradient needs -- "TT" (A and B row-contiguous: the score
terms) and "NT'" (A K-contiguous, B row-contiguous: the value terms) -- in bf16 and f32:

  1. against the float64 sum of the per-segment products (F32_TOL / BF16_TOL of tests/test_ops_gpu.py, repeated here because test
     modules do not import each other, applied as in tests/test_gemm_fine_tile_gpu.py::_cmp);
  2. one segment is bit-equal to bist_gemm of the same descriptor where that takes the 128-tile kernel;
  3. segments whose K_s are whole K tiles are bit-equal to one bist_gemm over the operands concatenated along K;
  4. two launches are bit-equal;
  5. a sentinel border (ldc > N, rows >= M) is untouched;
  6. bist_gemm_kseg_ok refuses what the LDS-DMA stager cannot address, and the wrapper then runs the products one by one.
"""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

F32_TOL = 2e-5
BF16_TOL = 1.2e-2
DTYPES = [(torch.float32, F32_TOL), (torch.bfloat16, BF16_TOL)]
LAYOUTS = ["TT", "NT"]          # A row-contiguous / K-contiguous; B row-contiguous in both


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from bist_amd import _lib, ops as o
    assert _lib.lib.bist_device_ok() == 1, _lib.lib.bist_last_error()
    assert o.GEMM_KSEG_MAX >= 24
    return o


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _cmp(got, ref, tol, what):
    got = got.detach().float().cpu().double()
    err = (got - ref).abs().max().item()
    scale = max(1.0, ref.abs().max().item())
    assert math.isfinite(err) and err <= tol * scale, f"{what}: max err {err:.3e} (scale {scale:.3e}, tol {tol})"


class Seg:
    """One segment: logical A [nb, M, K], B [nb or 1, N, K] (float64 of the rounded operands) and the device tensors in layout `lay`.
    b_shared: B has batch stride 0 (one weight for every batch entry)."""

    def __init__(self, ops, M, N, K, lay, dtype, nb, seed, b_shared=False, nsum=1):
        a = _rand(nb, M, K, seed=seed).to(dtype)
        b = (_rand(1 if b_shared else nb, N, K, seed=seed + 1000) * (K * nsum) ** -0.5).to(dtype)
        self.a64, self.b64 = a.double(), b.double()
        self.K = K
        if lay[0] == "N":       # A K-contiguous: [nb, M, K] as it is
            self.A, a_rs, a_ks, a_bs = a.cuda(), K, 1, M * K
        else:                   # A row-contiguous: stored [nb, K, M]  (the [B, R, TS] score gradients)
            self.A, a_rs, a_ks, a_bs = a.transpose(1, 2).contiguous().cuda(), 1, M, M * K
        self.B = b.transpose(1, 2).contiguous().cuda()          # stored [nb, K, N]
        b_bs = 0 if b_shared else N * K
        self.kw = dict(a_rs=a_rs, a_ks=a_ks, b_rs=1, b_ks=N, a_bs=(a_bs, 0), b_bs=(b_bs, 0))
        self.seg = ops.kseg(self.A, self.B, K, **self.kw)

    def product(self):
        return self.a64 @ self.b64.transpose(1, 2)


def _segments(ops, M, N, Ks, lay, dtype, nb=1, b_shared=False, seed=0):
    return [Seg(ops, M, N, K, lay, dtype, nb, seed + 7 * i, b_shared=b_shared, nsum=len(Ks)) for i, K in enumerate(Ks)]


def _run(ops, segs, M, N, dtype, nb=1, ldc=None, rows=None, **kw):
    """-> (output [nb, rows, ldc] with the sentinel 7 outside [M, N], the kseg launch's view of it)"""
    from bist_amd import _lib
    ldc, rows = ldc or N, rows or M
    out = torch.full((nb, rows, ldc), 7.0, device="cuda", dtype=dtype)
    g = ops.gemm_kseg_desc([s.seg for s in segs], out, M=M, N=N, ldc=ldc, batch=(nb, 1), c_bs=(rows * ldc, 0), **kw)
    assert _lib.lib.bist_gemm_kseg_ok(ctypes.byref(g)) == 1
    before = _lib.lib.bist_launch_count(_lib.K_GEMM_KSEG)
    _lib.check(_lib.lib.bist_gemm_kseg(ctypes.byref(g), torch.cuda.current_stream().cuda_stream), "bist_gemm_kseg")
    assert _lib.lib.bist_launch_count(_lib.K_GEMM_KSEG) == before + 1
    return out


def _ref(segs):
    return sum(s.product() for s in segs)


def _piece(dtype):
    return 16 // torch.empty((), dtype=dtype).element_size()


# (M, N, Ks, nb): every segment count, K_s, M, N and batch of the issue's table occurs in some case
SUM_CASES = [
    (200, 136, [8], 1),
    (200, 136, [64, 72], 3),
    (200, 512, [160, 160, 160], 1),
    (200, 136, [160, 512, 8, 72, 64], 3),
    (1568, 512, [160] * 12, 1),
    (200, 136, [72] * 24, 1),
    (1568, 136, [512, 64], 1),
]


@pytest.mark.parametrize("dtype,tol", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("lay", LAYOUTS)
@pytest.mark.parametrize("M,N,Ks,nb", SUM_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_sum_of_segments_against_float64(ops, dtype, tol, lay, M, N, Ks, nb):
    assert ops.GEMM_KSEG_MAX == 24 and M % _piece(dtype) == 0 and N % _piece(dtype) == 0
    if dtype == torch.float32 and 8 in Ks:
        Ks = Ks + [20]                                      # f32 also K_s = 20 (five 16-byte pieces), beside 8 (two pieces, a quarter tile)
    segs = _segments(ops, M, N, Ks, lay, dtype, nb=nb, b_shared=(nb > 1 and lay == "NT"))
    out = _run(ops, segs, M, N, dtype, nb=nb)
    ref = _ref(segs)
    _cmp(out, ref, tol, "plain")
    again = _run(ops, segs, M, N, dtype, nb=nb)
    assert torch.equal(_bits(out), _bits(again)), "two launches differ"
    if len(Ks) in (2, 5, 6):
        res = _rand(nb, M, N, seed=99).to(dtype)
        out = _run(ops, segs, M, N, dtype, nb=nb, alpha=0.5, residual=res.cuda(), ldr=N, r_bs=(M * N, 0))
        _cmp(out, 0.5 * ref + res.double(), tol, "alpha = 0.5 with residual")


@pytest.mark.parametrize("dtype,tol", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("lay", LAYOUTS)
def test_segments_with_different_batch_strides(ops, dtype, tol, lay):
    """[B, R, TS]-style and [B*TS, d]-style operands side by side: each segment brings its own batch strides; B with stride 0 and not"""
    M, N, nb = 200, 136, 3
    s0 = Seg(ops, M, N, 160, lay, dtype, nb, 1, nsum=3)
    s1 = Seg(ops, M, N, 72, lay, dtype, nb, 2, b_shared=True, nsum=3)
    # a third segment whose A lives inside a larger allocation with a padded batch stride
    s2 = Seg(ops, M, N, 64, lay, dtype, nb, 3, nsum=3)
    pad = 64
    big = torch.zeros(nb, s2.A[0].numel() + pad, device="cuda", dtype=dtype)
    big[:, :s2.A[0].numel()] = s2.A.reshape(nb, -1)
    kw = dict(s2.kw)
    kw["a_bs"] = (big.stride(0), 0)
    s2.seg = ops.kseg(big, s2.B, 64, **kw)
    out = _run(ops, [s0, s1, s2], M, N, dtype, nb=nb)
    _cmp(out, _ref([s0, s1, s2]), tol, "mixed batch strides")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("lay", LAYOUTS)
@pytest.mark.parametrize("K", [160, 512])
def test_one_segment_bits_equal_bist_gemm(ops, dtype, lay, K):
    """156 tiles of 128x128 (M = 1568, N = 512, batch 3): bist_gemm takes the 128-tile kernel, and one segment is that product"""
    from bist_amd import _lib
    M, N, nb = 1568, 512, 3
    s = Seg(ops, M, N, K, lay, dtype, nb, 5, b_shared=(lay == "NT"))
    out = _run(ops, [s], M, N, dtype, nb=nb)
    want = torch.empty(nb, M, N, device="cuda", dtype=dtype)
    g = ops.gemm_desc(s.A, s.B, want, M=M, N=N, K=K, ldc=N, batch=(nb, 1), c_bs=(M * N, 0), **s.kw)
    g.workspace, g.workspace_bytes = None, 0                          # no split-K (f32 at K = 512 is 16 K tiles on 156 output tiles)
    assert _lib.lib.bist_gemm_is_fast(ctypes.byref(g)) == 1          # the LDS-DMA tile kernel, no split-K, not the 256 tile
    _lib.check(_lib.lib.bist_gemm(ctypes.byref(g), torch.cuda.current_stream().cuda_stream), "bist_gemm")
    assert torch.equal(_bits(out), _bits(want))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("lay", LAYOUTS)
def test_whole_tile_segments_bits_equal_the_concatenated_product(ops, dtype, lay):
    """K_s in whole K tiles (64 bf16 / 32 f32 elements): the flat tile sequence is that of ONE product over [A_0 | A_1 | A_2]"""
    from bist_amd import _lib
    M, N, nb = 1568, 512, 3
    bk = 128 // torch.empty((), dtype=dtype).element_size()
    Ks = [bk, 3 * bk, 2 * bk]
    segs = _segments(ops, M, N, Ks, lay, dtype, nb=nb)
    out = _run(ops, segs, M, N, dtype, nb=nb)
    K = sum(Ks)
    a = torch.cat([s.a64 for s in segs], dim=2).to(dtype)         # [nb, M, K] (the operands are exactly representable: no re-rounding)
    b = torch.cat([s.b64 for s in segs], dim=2).to(dtype)
    A, a_rs, a_ks = (a.cuda(), K, 1) if lay[0] == "N" else (a.transpose(1, 2).contiguous().cuda(), 1, M)
    B = b.transpose(1, 2).contiguous().cuda()
    want = torch.empty(nb, M, N, device="cuda", dtype=dtype)
    g = ops.gemm_desc(A, B, want, M=M, N=N, K=K, a_rs=a_rs, a_ks=a_ks, b_rs=1, b_ks=N, ldc=N, batch=(nb, 1),
                      a_bs=(M * K, 0), b_bs=(N * K, 0), c_bs=(M * N, 0))
    g.workspace, g.workspace_bytes = None, 0
    assert _lib.lib.bist_gemm_is_fast(ctypes.byref(g)) == 1
    _lib.check(_lib.lib.bist_gemm(ctypes.byref(g), torch.cuda.current_stream().cuda_stream), "bist_gemm")
    assert torch.equal(_bits(out), _bits(want))


@pytest.mark.parametrize("dtype,tol", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("lay", LAYOUTS)
def test_border_is_untouched(ops, dtype, tol, lay):
    M, N, nb, ldc, rows = 200, 136, 3, 144, 208
    segs = _segments(ops, M, N, [72, 160], lay, dtype, nb=nb)
    out = _run(ops, segs, M, N, dtype, nb=nb, ldc=ldc, rows=rows)
    _cmp(out[:, :M, :N], _ref(segs), tol, "inside")
    o = out.float().cpu()
    assert (o[:, M:, :] == 7.0).all() and (o[:, :, N:] == 7.0).all(), "the launch wrote outside [M, N]"


def test_f32_output_from_bf16_operands(ops):
    M, N = 200, 136
    segs = _segments(ops, M, N, [160, 72, 8], "TT", torch.bfloat16)
    out = torch.full((1, M, N), 7.0, device="cuda", dtype=torch.float32)
    ops.gemm_kseg([s.seg for s in segs], out, M=M, N=N, ldc=N, batch=(1, 1), c_bs=(M * N, 0))
    _cmp(out, _ref(segs), 2e-3, "f32 output from bf16 operands")        # the bound tests/test_gemm_fine_tile_gpu.py uses for this epilogue


@pytest.mark.parametrize("dtype,tol", DTYPES, ids=["f32", "bf16"])
def test_one_segment_more_than_a_launch_holds_is_chained(ops, dtype, tol):
    from bist_amd import _lib
    M, N = 200, 136
    n = ops.GEMM_KSEG_MAX + 1
    segs = _segments(ops, M, N, [72] * n, "TT", dtype)
    out = torch.full((1, M, N), 7.0, device="cuda", dtype=dtype)
    assert not ops.gemm_kseg_ok([s.seg for s in segs], out, M=M, N=N, ldc=N)
    g = ops.gemm_kseg_desc([s.seg for s in segs[:-1]], out, M=M, N=N, ldc=N)
    g.nseg = n
    assert _lib.lib.bist_gemm_kseg_ok(ctypes.byref(g)) == 0
    assert _lib.lib.bist_gemm_kseg(ctypes.byref(g), torch.cuda.current_stream().cuda_stream) != 0      # refused, nothing launched
    before = _lib.lib.bist_launch_count(_lib.K_GEMM_KSEG)
    ops.gemm_kseg([s.seg for s in segs], out, M=M, N=N, ldc=N)
    assert _lib.lib.bist_launch_count(_lib.K_GEMM_KSEG) == before + 2
    _cmp(out, _ref(segs), tol, "chained through the residual")


@pytest.mark.parametrize("dtype,tol", DTYPES, ids=["f32", "bf16"])
def test_refused_descriptors_take_the_per_product_path(ops, dtype, tol):
    from bist_amd import _lib
    M, N = 200, 136
    p = _piece(dtype)
    kw = dict(M=M, N=N, ldc=N)
    out = torch.full((1, M, N), 7.0, device="cuda", dtype=dtype)
    good = _segments(ops, M, N, [72, 64], "NT", dtype)
    assert ops.gemm_kseg_ok([s.seg for s in good], out, **kw)

    def refused(segs, what, M_=M, out_=out):
        kw_ = dict(M=M_, N=N, ldc=N)
        assert not ops.gemm_kseg_ok(segs, out_, **kw_), what
        before = _lib.lib.bist_launch_count(_lib.K_GEMM_KSEG)
        ops.gemm_kseg(segs, out_, **kw_)
        assert _lib.lib.bist_launch_count(_lib.K_GEMM_KSEG) == before, what
        return out_

    # a misaligned base: A starts one element into its allocation
    s = good[0]
    flat = torch.zeros(s.A.numel() + p, device="cuda", dtype=dtype)
    flat[1:1 + s.A.numel()] = s.A.reshape(-1)
    mis = ops.kseg(flat, s.B, s.K, a_off=1, **s.kw)
    _cmp(refused([mis, good[1].seg], "misaligned base"), _ref(good), tol, "misaligned base")

    # a K-contiguous operand whose K_s is not whole 16-byte pieces
    odd = Seg(ops, M, N, 72 + p // 2, "NT", dtype, 1, 11, nsum=2)
    _cmp(refused([good[0].seg, odd.seg], "K_s not whole pieces"), _ref([good[0], odd]), tol, "K_s not whole pieces")

    # a row-contiguous operand whose row count is not whole pieces
    M2 = M + p // 2
    tt = _segments(ops, M2, N, [72, 64], "TT", dtype, seed=40)
    out2 = torch.full((1, M2, N), 7.0, device="cuda", dtype=dtype)
    _cmp(refused([s_.seg for s_ in tt], "rows not whole pieces", M_=M2, out_=out2), _ref(tt), tol, "rows not whole pieces")

    # segments of two layouts in one list
    mixed = [good[0], _segments(ops, M, N, [64], "TT", dtype, seed=50)[0]]
    _cmp(refused([s_.seg for s_ in mixed], "mixed layouts"), _ref(mixed), tol, "mixed layouts")
