"""bist_switch_logits_fwd / _bwd with FIVE parts (the modality fusion with audio: query, cap, spatial, temporal, audio -> four logits,
model/decoder.py:148-155) through the C ABI against a float64 host computation of the concatenated product: forward, the parts'
gradients with and without residual operands, dW / db written and accumulated, the border of a wider dW, two launches bit for bit.

Bounds are those of the same quantities elsewhere in the suite, with tol = 1e-5 (f32) or 2e-2 (bf16):
  logits          tol max(1, |ref|max)                      tests/test_train_gpu.py:1021
  parts' gradient tol max(1, |ref|max)                      tests/test_switch_logits_wgrad_gpu.py:79-82 (test_train_gpu.py:1023)
  dW              2 tol max(1, |ref|max), the bf16 figure as soon as operands or dW are bf16      test_switch_logits_wgrad_gpu.py:66, 76
  db              2 tol max(1, |ref|max) by the operand dtype (db is always f32)                   test_switch_logits_wgrad_gpu.py:77
The reference is computed from the values as the kernel reads them (operands rounded to their storage dtype), once per case.

Calls with <= 4 parts must compute what they computed before the limit was raised: for (d, n_parts, ns) = (512, 4, 3) the outputs of
``_record_case`` equal, bit for bit, tests/golden/g9_switch_logits4_parent.npz -- the outputs of this very function run against the
library built from the commit before the change (python tests/test_switch_logits5_gpu.py LIBRARY OUT.npz loads that library with ctypes
and writes the file; inputs come from a seeded host generator, so they are the same on both sides).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = [1, 7, 320]
GEOM = [(512, 5, 4), (64, 5, 4), (128, 5, 1), (512, 5, 3)]       # (d, n_parts, ns)
TOL = {torch.float32: 1e-5, torch.bfloat16: 2e-2}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g9_switch_logits4_parent.npz")


def _code(dtype):
    from bist_amd.ops import dtype_code
    return dtype_code(dtype)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _fwd(cdll, parts, w, bias, out, rows, d, ns):
    rc = cdll.bist_switch_logits_fwd(_ptrs(parts), len(parts), w.data_ptr(), w.stride(0), bias.data_ptr() if bias is not None else None,
                                     out.data_ptr(), _code(out.dtype), rows, d, ns, _code(w.dtype), _stream())
    assert rc == 0, cdll.bist_last_error()


def _bwd(cdll, parts, w, dsw, dparts, res, dW, lddw, acc_w, db, acc_b, rows, d, ns):
    rc = cdll.bist_switch_logits_bwd(_ptrs(parts), len(parts), w.data_ptr(), w.stride(0), dsw.data_ptr(), _code(dsw.dtype),
                                     _ptrs(dparts) if dparts is not None else None, _ptrs(res) if res is not None else None,
                                     dW.data_ptr() if dW is not None else None, lddw, _code(dW.dtype) if dW is not None else 0, acc_w,
                                     db.data_ptr() if db is not None else None, acc_b, rows, d, ns, _code(w.dtype), _stream())
    assert rc == 0, cdll.bist_last_error()


def _inputs(rows, d, n, ns, dtype):
    g = torch.Generator().manual_seed(5000 * rows + d + 7 * ns + n)
    parts = [torch.randn(rows, d, generator=g).to(dtype) for _ in range(n)]
    res = [torch.randn(rows, d, generator=g).to(dtype) for _ in range(n)]
    w = (torch.randn(ns, n * d, generator=g) * 0.1).to(dtype)
    bias = torch.randn(ns, generator=g).to(dtype)
    dsw = torch.randn(rows, ns, generator=g)
    dw0 = torch.randn(ns, n * d, generator=g)
    db0 = torch.randn(ns, generator=g)
    return parts, res, w, bias, dsw, dw0, db0


def _run_case(cdll, rows, d, n, ns, dtype):
    """Every output of one case as device tensors, in a fixed order of launches (also the body of the recording)."""
    parts, res, w, bias, dsw, dw0, db0 = _inputs(rows, d, n, ns, dtype)
    pd, rd, wd, bd, gd = [p.cuda() for p in parts], [r.cuda() for r in res], w.cuda(), bias.cuda(), dsw.cuda()
    out = {}
    for od in sorted({torch.float32, dtype}, key=str):
        o = torch.full((rows, ns), float("nan"), dtype=od).cuda()
        _fwd(cdll, pd, wd, bd, o, rows, d, ns)
        out[f"fwd_{od}"] = o
    o = torch.full((rows, ns), float("nan")).cuda()
    _fwd(cdll, pd, wd, None, o, rows, d, ns)
    out["fwd_nobias"] = o
    for name, r in (("dx", None), ("dx_res", rd), ("dx_res_some", [x if j % 2 == 0 else None for j, x in enumerate(rd)])):
        dps = [torch.full((rows, d), float("nan"), dtype=dtype).cuda() for _ in range(n)]
        _bwd(cdll, pd, wd, gd, dps, r, None, 0, 0, None, 0, rows, d, ns)
        for j, t in enumerate(dps):
            out[f"{name}{j}"] = t
    for dw_dtype in (torch.float32, torch.bfloat16):
        for acc in (0, 1):
            dW = dw0.to(dw_dtype).cuda() if acc else torch.full((ns, n * d), float("nan"), dtype=dw_dtype).cuda()
            db = db0.clone().cuda() if acc else torch.full((ns,), float("nan")).cuda()
            dps = [torch.empty(rows, d, dtype=dtype).cuda() for _ in range(n)] if acc else None        # with and without the parts branch
            _bwd(cdll, pd, wd, gd, dps, rd if acc else None, dW, n * d, acc, db, acc, rows, d, ns)
            out[f"dW_{dw_dtype}_{acc}"], out[f"db_{dw_dtype}_{acc}"] = dW, db
    torch.cuda.synchronize()
    return out, (parts, res, w, bias, dsw, dw0, db0)


@pytest.fixture(scope="module")
def cdll():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from bist_amd import _lib
    assert _lib.lib.bist_device_ok() == 1, _lib.lib.bist_last_error()
    return _lib.lib


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("d,n,ns", GEOM)
@pytest.mark.parametrize("rows", ROWS)
def test_five_parts_against_float64(cdll, rows, d, n, ns, dtype):
    got, (parts, res, w, bias, dsw, dw0, db0) = _run_case(cdll, rows, d, n, ns, dtype)
    tol = TOL[dtype]
    sc = lambda t: max(1.0, t.abs().max().item())
    err = lambda a, b: (a.double().cpu() - b).abs().max().item()
    x6, w6, g6 = torch.cat([p.double() for p in parts], -1), w.double(), dsw.double()
    ref = x6 @ w6.t()
    for k in [k for k in got if k.startswith("fwd_torch")]:
        assert err(got[k], ref + bias.double()) <= tol * sc(ref + bias.double()), k
    assert err(got["fwd_nobias"], ref) <= tol * sc(ref)
    ref_x = g6 @ w6
    for j in range(n):
        rj = ref_x[:, j * d:(j + 1) * d]
        assert err(got[f"dx{j}"], rj) <= tol * sc(rj), j
        rr = rj + res[j].double()
        assert err(got[f"dx_res{j}"], rr) <= tol * sc(rr), j
        rs = rr if j % 2 == 0 else rj
        assert err(got[f"dx_res_some{j}"], rs) <= tol * sc(rs), j
    ref_w, ref_b = g6.t() @ x6, g6.sum(0)
    for dw_dtype in (torch.float32, torch.bfloat16):
        tw = 1e-5 if (dtype == torch.float32 and dw_dtype == torch.float32) else 2e-2
        for acc in (0, 1):
            want_w = ref_w + (dw0.to(dw_dtype).double() if acc else 0.0)
            want_b = ref_b + (db0.double() if acc else 0.0)
            assert err(got[f"dW_{dw_dtype}_{acc}"], want_w) <= 2 * tw * sc(want_w), (dw_dtype, acc)
            assert err(got[f"db_{dw_dtype}_{acc}"], want_b) <= 2 * tol * sc(want_b), (dw_dtype, acc)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,d,n,ns", [(320, 512, 5, 4), (7, 64, 5, 4), (1, 128, 5, 1)])
def test_two_calls_give_identical_bits(cdll, rows, d, n, ns, dtype):
    """deterministic=True rests on this: no atomics, no order that depends on arrival."""
    a, _ = _run_case(cdll, rows, d, n, ns, dtype)
    b, _ = _run_case(cdll, rows, d, n, ns, dtype)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("dtype,dw_dtype", [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.bfloat16, torch.float32)])
@pytest.mark.parametrize("rows,d,n,ns", [(7, 64, 5, 4), (320, 512, 5, 3)])
def test_a_wider_weight_gradient_keeps_its_border(cdll, rows, d, n, ns, dtype, dw_dtype):
    """lddw larger than n_parts d: the border of dW keeps its poison, for both accumulate forms; rows past ns too."""
    parts, res, w, bias, dsw, dw0, db0 = _inputs(rows, d, n, ns, dtype)
    pd, wd, gd = [p.cuda() for p in parts], w.cuda(), dsw.cuda()
    pad, poison = 24, 96.0                                 # exact in bf16
    ref = dsw.double().t() @ torch.cat([p.double() for p in parts], -1)
    tol = 1e-5 if dw_dtype == torch.float32 and dtype == torch.float32 else 2e-2
    for acc in (0, 1):
        buf = torch.full((ns + 1, n * d + pad), poison, dtype=dw_dtype).cuda()
        db = torch.zeros(ns).cuda()
        _bwd(cdll, pd, wd, gd, None, None, buf, n * d + pad, acc, db, 0, rows, d, ns)
        out = buf.double().cpu()
        assert (out[:ns, n * d:] == poison).all() and (out[ns] == poison).all(), acc
        want = ref + (poison if acc else 0.0)
        assert (out[:ns, :n * d] - want).abs().max().item() <= 2 * tol * max(1.0, want.abs().max().item()), acc


def test_six_parts_are_refused(cdll):
    parts = [torch.zeros(4, 64).cuda() for _ in range(6)]
    w, out = torch.zeros(2, 6 * 64).cuda(), torch.zeros(4, 2).cuda()
    rc = cdll.bist_switch_logits_fwd(_ptrs(parts), 6, w.data_ptr(), w.stride(0), None, out.data_ptr(), _code(out.dtype), 4, 64, 2,
                                     _code(w.dtype), _stream())
    assert rc != 0 and b"1..5 parts" in cdll.bist_last_error()


def _record_case(cdll):
    """(512, 4, 3) at every row count and dtype -> {name: the SHA-256 of the output's bytes as 32 uint8} (the outputs themselves are
    megabytes; equal digests are equal bits); the logits and db, which are small, are kept as they are too (bf16 as its 16-bit words)."""
    import hashlib
    rec = {}
    for rows in ROWS:
        for dtype in (torch.float32, torch.bfloat16):
            got, _ = _run_case(cdll, rows, 512, 4, 3, dtype)
            for k, t in got.items():
                t = t.cpu().contiguous()
                raw = t.view(torch.int16).numpy() if t.dtype == torch.bfloat16 else t.numpy()
                name = f"r{rows}_{str(dtype).split('.')[-1]}_{k}"
                rec["sha_" + name] = np.frombuffer(hashlib.sha256(raw.tobytes()).digest(), dtype=np.uint8).copy()
                if k.startswith("fwd") or k.startswith("db"):
                    rec["raw_" + name] = raw
    return rec


def test_four_parts_equal_the_recording_of_the_commit_before(cdll):
    want = np.load(GOLDEN)
    got = _record_case(cdll)
    assert sorted(got) == sorted(want.files)
    for k in sorted(got, key=lambda k: (not k.startswith("raw_"), k)):          # the small raw outputs first: a mismatch there shows values
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), k


if __name__ == "__main__":
    # python tests/test_switch_logits5_gpu.py LIBRARY OUT.npz : record _record_case() from another build of the library
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bist_amd import _lib
    other = C.CDLL(os.path.abspath(sys.argv[1]))
    for name in ("bist_switch_logits_fwd", "bist_switch_logits_bwd", "bist_last_error"):
        fn = getattr(other, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    np.savez_compressed(sys.argv[2], **_record_case(other))
    print("recorded", sys.argv[2], os.path.getsize(sys.argv[2]) // 1024, "KiB")
