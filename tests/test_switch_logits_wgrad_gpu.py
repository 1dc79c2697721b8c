"""The weight / bias gradient of the fusion logits (bist_switch_logits_bwd, weights branch) through the C ABI against float64:
sixteen row slices per workgroup that meet in LDS, 4-byte column pieces, one writer per dW / db element.  Row counts below, at and
above the slice count and the 16-row step, ragged classes with more than 320 rows, every dtype combination the entry accepts, both
accumulate forms, with and without the parts branch in the same call.

Tolerance: that of test_switch_logits_launch_forward_and_backward -- 2 tol max(1, |ref|max) with tol = 1e-5 (f32) or 2e-2 (bf16).  A
gradient STORED in bf16 carries bf16's rounding (2^-9 relative) whatever the operands are, so the bf16 figure applies as soon as the
operands or dW are bf16.  The reference is computed from the values as the kernel reads them (operands and dsw rounded to their
storage dtype), once per case, and shared by the sixteen launches of the case."""
import ctypes as C
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = [1, 5, 37, 320, 333, 1283]
GEOM = [(512, 4, 3), (64, 3, 1), (128, 1, 4), (512, 2, 2)]       # (d, n_parts, ns)


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from bist_amd import _lib
    assert _lib.lib.bist_device_ok() == 1, _lib.lib.bist_last_error()
    return _lib


def _launch(lib, parts, w, dsw, dparts, dW, lddw, acc_w, db, acc_b, rows, d, ns):
    from bist_amd.ops import dtype_code
    n = len(parts)
    arr = (C.c_void_p * n)(*[p.data_ptr() for p in parts])
    darr = (C.c_void_p * n)(*[p.data_ptr() for p in dparts]) if dparts is not None else None
    lib.check(lib.lib.bist_switch_logits_bwd(arr, n, w.data_ptr(), w.stride(0), dsw.data_ptr(), dtype_code(dsw.dtype), darr, None,
                                             dW.data_ptr(), lddw, dtype_code(dW.dtype), acc_w, db.data_ptr(), acc_b, rows, d, ns,
                                             dtype_code(w.dtype), torch.cuda.current_stream().cuda_stream), "bist_switch_logits_bwd")


def _inputs(rows, d, n, ns, dtype):
    g = torch.Generator().manual_seed(1000 * rows + d + ns)
    parts = [torch.randn(rows, d, generator=g).to(dtype) for _ in range(n)]
    w = (torch.randn(ns, n * d, generator=g) * 0.1).to(dtype)
    dsw = torch.randn(rows, ns, generator=g)
    dw0 = torch.randn(ns, n * d, generator=g)
    db0 = torch.randn(ns, generator=g)
    return parts, w, dsw, dw0, db0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("d,n,ns", GEOM)
@pytest.mark.parametrize("rows", ROWS)
def test_weight_and_bias_gradient_against_float64(lib, rows, d, n, ns, dtype):
    parts, w, dsw, dw0, db0 = _inputs(rows, d, n, ns, dtype)
    pd, wd = [p.cuda() for p in parts], w.cuda()
    x6 = torch.cat([p.double() for p in parts], -1)
    sc = lambda t: max(1.0, t.abs().max().item())
    dsw_dtypes = [torch.float32] if dtype == torch.float32 else [torch.float32, dtype]
    for dsw_dtype in dsw_dtypes:
        dswd = dsw.to(dsw_dtype).cuda()
        g6 = dsw.to(dsw_dtype).double()
        ref_w, ref_b = g6.t() @ x6, g6.sum(0)                    # once per (case, dsw dtype)
        ref_x = g6 @ w.double()
        for dw_dtype, acc, with_parts in itertools.product([torch.float32, torch.bfloat16], [0, 1], [False, True]):
            tol = 1e-5 if (dtype == torch.float32 and dw_dtype == torch.float32) else 2e-2
            what = (str(dsw_dtype), str(dw_dtype), acc, with_parts)
            dW = dw0.to(dw_dtype).cuda() if acc else torch.full((ns, n * d), float("nan"), dtype=dw_dtype).cuda()
            db = db0.clone().cuda() if acc else torch.full((ns,), float("nan")).cuda()
            dparts = [torch.empty_like(p) for p in pd] if with_parts else None
            _launch(lib, pd, wd, dswd, dparts, dW, n * d, acc, db, acc, rows, d, ns)
            want_w = ref_w + (dw0.to(dw_dtype).double() if acc else 0.0)
            want_b = ref_b + (db0.double() if acc else 0.0)
            err_w = (dW.double().cpu() - want_w).abs().max().item()
            err_b = (db.double().cpu() - want_b).abs().max().item()
            assert err_w <= 2 * tol * sc(want_w), (what, err_w)
            assert err_b <= 2 * (1e-5 if dtype == torch.float32 else 2e-2) * sc(want_b), (what, err_b)      # db is always f32
            if with_parts:
                tol_x = 1e-5 if dtype == torch.float32 else 2e-2
                for j in range(n):
                    rj = ref_x[:, j * d:(j + 1) * d]
                    assert (dparts[j].double().cpu() - rj).abs().max().item() <= tol_x * sc(rj), (what, j)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,d,n,ns", [(320, 512, 4, 3), (333, 512, 2, 2), (1283, 128, 1, 4), (5, 64, 3, 1)])
def test_two_launches_give_the_same_bits(lib, rows, d, n, ns, dtype):
    """No atomics and nothing between workgroups: the order of every sum follows from (rows, d, n_parts, ns) alone."""
    parts, w, dsw, dw0, db0 = _inputs(rows, d, n, ns, dtype)
    pd, wd, dswd = [p.cuda() for p in parts], w.cuda(), dsw.cuda()
    for acc in (0, 1):
        got = []
        for rep in range(2):
            dW, db = dw0.clone().cuda(), db0.clone().cuda()
            _launch(lib, pd, wd, dswd, None, dW, n * d, acc, db, acc, rows, d, ns)
            got.append((dW, db))
        assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]), acc


@pytest.mark.parametrize("dtype,dw_dtype", [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.bfloat16, torch.float32)])
@pytest.mark.parametrize("rows,d,n,ns", [(37, 64, 3, 1), (320, 512, 4, 3), (5, 128, 1, 4)])
def test_columns_past_the_parts_stay_untouched(lib, rows, d, n, ns, dtype, dw_dtype):
    """lddw larger than n_parts d: the border of dW keeps its poison, for both accumulate forms; rows past ns too."""
    parts, w, dsw, dw0, db0 = _inputs(rows, d, n, ns, dtype)
    pd, wd, dswd = [p.cuda() for p in parts], w.cuda(), dsw.cuda()
    pad, poison = 24, 96.0                                 # exact in bf16
    ref = dsw.double().t() @ torch.cat([p.double() for p in parts], -1)
    tol = 1e-5 if dw_dtype == torch.float32 and dtype == torch.float32 else 2e-2
    for acc in (0, 1):
        buf = torch.full((ns + 1, n * d + pad), poison, dtype=dw_dtype).cuda()
        db = torch.zeros(ns).cuda()
        _launch(lib, pd, wd, dswd, None, buf, n * d + pad, acc, db, 0, rows, d, ns)
        out = buf.double().cpu()
        assert (out[:ns, n * d:] == poison).all() and (out[ns] == poison).all(), acc
        want = ref + (poison if acc else 0.0)
        assert (out[:ns, :n * d] - want).abs().max().item() <= 2 * tol * max(1.0, want.abs().max().item()), acc
