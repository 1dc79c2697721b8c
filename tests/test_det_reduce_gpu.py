"""The deterministic reductions of det_reduce.hip at the C ABI: column sums (bias gradients), LayerNorm gain / offset gradients, the
stage-2 value bias and the shared embedding, fp32 and bf16.

Accuracy bounds are the worst case of ANY fp32 summation order, n * 2^-23 * sum|terms| against an fp64 sum of the same (already
rounded) inputs -- derived, not tuned.  Reproducibility is bit equality: over repeats (some beside a second stream that copies
unrelated memory), and of one job alone against the same job inside a launch of many."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23
DTYPES = [torch.float32, torch.bfloat16]


def _lib():
    from bist_amd import _lib
    return _lib


def _code(dt):
    from bist_amd.ops import dtype_code
    return dtype_code(dt)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _wide(shape, gen, lo=-3.0, hi=3.0):
    """randn * 10^U(lo, hi): magnitudes over several decades, so that the order of an fp32 sum shows in its bits."""
    return torch.randn(shape, generator=gen, device="cuda") * 10.0 ** (torch.rand(shape, generator=gen, device="cuda") * (hi - lo) + lo)


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _repeat(run, n=8):
    """run() -> tensors; n runs, the odd ones beside a second stream that copies unrelated memory; every run must equal the first."""
    first = [t.clone() for t in run()]
    side = torch.cuda.Stream()
    src = torch.randn(1 << 22, device="cuda")
    dst = torch.empty_like(src)
    for i in range(1, n):
        if i % 2:
            with torch.cuda.stream(side):
                for _ in range(4):
                    dst.copy_(src)
        got = run()
        torch.cuda.synchronize()
        for a, b in zip(first, got):
            assert torch.equal(a, b), "repeat %d differs" % i
    return first


# ---- column sums ---------------------------------------------------------------------------------------------------------------------
def _col_jobs(specs, dtype, seed):
    g = _gen(seed)
    return [_wide((M, N), g).to(dtype) for M, N in specs]


def _col_sum(xs, outs, ws=None, ws_bytes=None):
    L = _lib()
    arr = (L.BistColSum * len(xs))()
    for i, (x, o) in enumerate(zip(xs, outs)):
        arr[i].x, arr[i].out, arr[i].M, arr[i].N, arr[i].ldx = x.data_ptr(), o.data_ptr(), x.shape[0], x.shape[1], x.stride(0)
    need = L.lib.bist_col_sum_multi_det_workspace(arr, len(xs))
    assert need > 0
    if ws is None:
        ws = torch.empty(need // 4, device="cuda", dtype=torch.float32)
    rc = L.lib.bist_col_sum_multi_det(arr, len(xs), _code(xs[0].dtype), ws.data_ptr(), ws.numel() * 4 if ws_bytes is None else ws_bytes, _stream())
    return rc, need


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("M,N", [(200, 96), (203, 130)], ids=["vector", "scalar-ragged"])
def test_col_sum_bound_repeats_batching_and_accumulation(M, N, dtype):
    (x,) = _col_jobs([(M, N)], dtype, 1)

    def run():
        out = torch.zeros(N, device="cuda")
        rc, _ = _col_sum([x], [out])
        assert rc == 0, _lib().lib.bist_last_error()
        return [out]
    (alone,) = _repeat(run)
    ref = x.double().sum(0)
    bound = M * EPS32 * x.double().abs().sum(0)
    err = (alone.double() - ref).abs()
    print("col sum %s [%d x %d]: max err / bound %.3f" % (dtype, M, N, (err / bound).max().item()))
    assert (err <= bound).all()
    # the same job as job 17 of 40 mixed jobs: one chunk to many, scalar and vector widths
    specs = [(1 + (37 * i) % 300, 8 + (29 * i) % 200) for i in range(40)]
    xs = _col_jobs(specs, dtype, 2)
    xs[17] = x
    outs = [torch.zeros(t.shape[1], device="cuda") for t in xs]
    rc, _ = _col_sum(xs, outs)
    assert rc == 0, _lib().lib.bist_last_error()
    torch.cuda.synchronize()
    assert torch.equal(outs[17], alone)
    for t, o in zip(xs, outs):            # and every other job of the launch is a column sum too
        assert ((o.double() - t.double().sum(0)).abs() <= t.shape[0] * EPS32 * t.double().abs().sum(0)).all()
    # accumulation into a non-zero destination: one plain add of the job's total
    out0 = torch.randn(N, device="cuda")
    out = out0.clone()
    rc, _ = _col_sum([x], [out])
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(out, out0 + alone)


# ---- LayerNorm gain / offset gradients ----------------------------------------------------------------------------------------------
def _ln_inputs(rows, d, dtype, seed):
    g = _gen(seed)
    x = (torch.randn((rows, d), generator=g, device="cuda") * 2.0 + 0.5).to(dtype)
    # two decades: enough for the order to show in the bits, while every column still has several rows that carry its sum -- the bound
    # below is relative to sum|term| of the column, and the fp32 mean of a row is only good to ~1e-8 absolute
    dy = _wide((rows, d), g, -1.0, 1.0).to(dtype)
    a = torch.ones(d, device="cuda", dtype=dtype)
    return dy, x, a


def _ln_grad(jobs, d, eps=1e-6):
    """jobs: (dy, x, a, da, db)"""
    L = _lib()
    arr = (L.BistLnGrad * len(jobs))()
    for i, (dy, x, a, da, db) in enumerate(jobs):
        arr[i].dy, arr[i].x, arr[i].a, arr[i].da, arr[i].db = dy.data_ptr(), x.data_ptr(), a.data_ptr(), da.data_ptr(), db.data_ptr()
        arr[i].rows, arr[i].lddy, arr[i].ldx, arr[i].eps = x.shape[0], dy.stride(0), x.stride(0), eps
    need = L.lib.bist_layernorm_param_grad_multi_det_workspace(arr, len(jobs), d)
    assert need > 0
    ws = torch.empty(need // 4, device="cuda", dtype=torch.float32)
    return L.lib.bist_layernorm_param_grad_multi_det(arr, len(jobs), d, _code(jobs[0][0].dtype), ws.data_ptr(), need, _stream())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,d", [(200, 64), (37, 512)])
def test_layernorm_param_grads_bound_repeats_and_batching(rows, d, dtype):
    dy, x, a = _ln_inputs(rows, d, dtype, 3)
    eps = 1e-6

    def run():
        da, db = torch.zeros(d, device="cuda"), torch.zeros(d, device="cuda")
        assert _ln_grad([(dy, x, a, da, db)], d, eps) == 0, _lib().lib.bist_last_error()
        return [da, db]
    da, db = _repeat(run)
    xd, gd = x.double(), dy.double()
    xc = xd - xd.mean(1, keepdim=True)
    term = gd * xc / (xd.std(1, keepdim=True) + eps)          # unbiased std, eps outside the root (modules.py:28-31)
    ea, eb = (da.double() - term.sum(0)).abs(), (db.double() - gd.sum(0)).abs()
    ba, bb = rows * EPS32 * term.abs().sum(0), rows * EPS32 * gd.abs().sum(0)
    print("ln grads %s [%d x %d]: max err / bound da %.3f db %.3f" % (dtype, rows, d, (ea / ba).max().item(), (eb / bb).max().item()))
    assert (ea <= ba).all() and (eb <= bb).all()
    # as job 17 of 40 jobs of the same width and other row counts
    jobs = []
    for i in range(40):
        r = 1 + (53 * i) % 700
        jdy, jx, ja = _ln_inputs(r, d, dtype, 100 + i)
        jobs.append((jdy, jx, ja, torch.zeros(d, device="cuda"), torch.zeros(d, device="cuda")))
    jobs[17] = (dy, x, a, torch.zeros(d, device="cuda"), torch.zeros(d, device="cuda"))
    assert _ln_grad(jobs, d, eps) == 0, _lib().lib.bist_last_error()
    torch.cuda.synchronize()
    assert torch.equal(jobs[17][3], da) and torch.equal(jobs[17][4], db)
    # accumulation
    a0, b0 = torch.randn(d, device="cuda"), torch.randn(d, device="cuda")
    a1, b1 = a0.clone(), b0.clone()
    assert _ln_grad([(dy, x, a, a1, b1)], d, eps) == 0
    torch.cuda.synchronize()
    assert torch.equal(a1, a0 + da) and torch.equal(b1, b0 + db)


# ---- stage-2 value bias -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_scaled_bias_bwd_ds_bitwise_dbias_bound_and_repeats(dtype):
    L = _lib()
    M, h, dk, nsets = 32, 4, 16, 2
    d, Mset = h * dk, M // nsets
    g = _gen(5)
    dy = _wide((M, d), g).to(dtype)
    s = torch.rand((M, h), generator=g, device="cuda") + 0.5
    bias = torch.randn((nsets, d), generator=g, device="cuda").to(dtype)
    need = L.lib.bist_scaled_bias_bwd_det_workspace(M, h, dk, nsets)
    assert need > 0
    ws = torch.empty(need // 4, device="cuda", dtype=torch.float32)

    def run():
        ds, db = torch.empty((M, h), device="cuda"), torch.zeros((nsets, d), device="cuda")
        rc = L.lib.bist_scaled_bias_bwd_det(dy.data_ptr(), s.data_ptr(), bias.data_ptr(), ds.data_ptr(), db.data_ptr(), M, h, dk, nsets, d, d,
                                            _code(dtype), ws.data_ptr(), need, _stream())
        assert rc == 0, L.lib.bist_last_error()
        return [ds, db]
    ds, db = _repeat(run)
    ds0, db0 = torch.empty((M, h), device="cuda"), torch.zeros((nsets, d), device="cuda")
    assert L.lib.bist_scaled_bias_bwd_z(dy.data_ptr(), s.data_ptr(), bias.data_ptr(), ds0.data_ptr(), db0.data_ptr(), M, h, dk, nsets, d, d,
                                        _code(dtype), _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(ds, ds0)
    term = (s.double().repeat_interleave(dk, 1) * dy.double()).view(nsets, Mset, d)
    err, bound = (db.double() - term.sum(1)).abs(), Mset * EPS32 * term.abs().sum(1)
    print("scaled bias %s: max err / bound %.3f" % (dtype, (err / bound).max().item()))
    assert (err <= bound).all()
    db1 = torch.ones((nsets, d), device="cuda")            # accumulates
    ds1 = torch.empty((M, h), device="cuda")
    assert L.lib.bist_scaled_bias_bwd_det(dy.data_ptr(), s.data_ptr(), bias.data_ptr(), ds1.data_ptr(), db1.data_ptr(), M, h, dk, nsets, d, d,
                                          _code(dtype), ws.data_ptr(), need, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(db1, torch.ones_like(db) + db)


# ---- embedding -------------------------------------------------------------------------------------------------------------------------
V, D = 80, 64
EMB_ROWS = (32, 48, 8)


def _emb_jobs(dtype, seed):
    """Three jobs over a pool of 11 of the 80 ids: every id of the pool occurs several times and in more than one job."""
    g = _gen(seed)
    pool = torch.tensor([0, 3, 7, 12, 20, 33, 41, 56, 63, 78, 79], device="cuda")
    jobs = []
    for k, rows in enumerate(EMB_ROWS):
        idx = (torch.arange(rows, device="cuda") * (k + 2) + k) % len(pool)      # walks the whole pool in every job (8 rows: 8 of the 11)
        idx[rows // 2:] = torch.randint(0, len(pool), (rows - rows // 2,), generator=g, device="cuda")
        jobs.append((pool[idx].contiguous(), _wide((rows, D), g).to(dtype)))
    return jobs


def _embed_det(jobs, dlut, drop=None):
    L = _lib()
    arr = (L.BistEmbedBwd * len(jobs))()
    for i, (ids, dy) in enumerate(jobs):
        arr[i].ids, arr[i].dy, arr[i].rows = ids.data_ptr(), dy.data_ptr(), ids.numel()
        arr[i].drop = L.BistDrop(drop[0], drop[1] + i, None) if drop else L.BistDrop(0.0, 0, None)
    return L.lib.bist_embed_bwd_multi_det(arr, len(jobs), dlut.data_ptr(), dlut.shape[0], D, _code(jobs[0][1].dtype), _stream())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_embedding_equals_the_specified_order_without_dropout(dtype):
    jobs = _emb_jobs(dtype, 7)
    all_ids = torch.cat([j[0] for j in jobs])
    counts = torch.bincount(all_ids, minlength=V)
    assert (counts[counts > 0] >= 3).all()
    for i in set(all_ids.tolist()):
        assert sum(bool((j[0] == i).any()) for j in jobs) >= 2, i
    base = torch.randn((V, D), generator=_gen(8), device="cuda")

    def run():
        dlut = base.clone()
        assert _embed_det(jobs, dlut) == 0, _lib().lib.bist_last_error()
        return [dlut]
    (got,) = _repeat(run)
    # the specified order on the CPU in fp32: per id, rows in ascending global order into a zero accumulator, then one add
    ids_c = all_ids.cpu().tolist()
    g = torch.cat([j[1] for j in jobs]).float().cpu() * torch.tensor(float(D)).sqrt()
    want = base.cpu().clone()
    for i in sorted(set(ids_c)):
        acc = torch.zeros(D)
        for r, v in enumerate(ids_c):
            if v == i:
                acc = acc + g[r]
        want[i] = want[i] + acc
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_embedding_with_dropout_matches_the_atomic_kernel_within_the_bound(dtype):
    L = _lib()
    jobs = _emb_jobs(dtype, 9)
    p, seed = 0.25, 1234

    def run():
        dlut = torch.zeros((V, D), device="cuda")
        assert _embed_det(jobs, dlut, (p, seed)) == 0, L.lib.bist_last_error()
        return [dlut]
    (got,) = _repeat(run)
    ref = torch.zeros((V, D), device="cuda")
    for i, (ids, dy) in enumerate(jobs):
        dr = L.BistDrop(p, seed + i, None)
        assert L.lib.bist_embed_bwd(ids.data_ptr(), dy.data_ptr(), ref.data_ptr(), ids.numel(), D, C.byref(dr), _code(dtype), _stream()) == 0
    plain = torch.zeros((V, D), device="cuda")
    assert _embed_det(jobs, plain) == 0
    torch.cuda.synchronize()
    all_ids = torch.cat([j[0] for j in jobs])
    mag = torch.zeros((V, D), device="cuda", dtype=torch.float64)
    mag.index_add_(0, all_ids, torch.cat([j[1] for j in jobs]).double().abs() * (D ** 0.5) / (1.0 - p))      # >= sum|kept terms|
    n = torch.bincount(all_ids, minlength=V).double().unsqueeze(1)
    err = (got.double() - ref.double()).abs()
    assert (err <= n * EPS32 * mag).all()
    assert not torch.equal(got, plain)            # the mask was applied
    assert (got[mag.sum(1) == 0] == 0).all()      # ids nobody carries stay untouched


# ---- refusal ---------------------------------------------------------------------------------------------------------------------------
def test_an_undersized_workspace_is_refused_and_nothing_is_launched():
    L = _lib()
    (x,) = _col_jobs([(200, 96)], torch.float32, 11)
    out = torch.full((96,), 3.0, device="cuda")
    ws = torch.empty(1 << 16, device="cuda", dtype=torch.float32)
    rc, need = _col_sum([x], [out], ws=ws, ws_bytes=0)
    assert need == 13 * 96 * 4                       # 200 rows in chunks of 16
    rc, _ = _col_sum([x], [out], ws=ws, ws_bytes=need - 4)
    assert rc != 0 and b"workspace" in L.lib.bist_last_error()
    dy, xx, a = _ln_inputs(37, 64, torch.float32, 12)
    da, db = torch.full((64,), 3.0, device="cuda"), torch.full((64,), 3.0, device="cuda")
    arr = (L.BistLnGrad * 1)()
    arr[0].dy, arr[0].x, arr[0].a, arr[0].da, arr[0].db = dy.data_ptr(), xx.data_ptr(), a.data_ptr(), da.data_ptr(), db.data_ptr()
    arr[0].rows, arr[0].lddy, arr[0].ldx, arr[0].eps = 37, 64, 64, 1e-6
    need = L.lib.bist_layernorm_param_grad_multi_det_workspace(arr, 1, 64)
    assert L.lib.bist_layernorm_param_grad_multi_det(arr, 1, 64, _code(torch.float32), ws.data_ptr(), need - 4, _stream()) != 0
    need = L.lib.bist_scaled_bias_bwd_det_workspace(32, 4, 16, 2)
    ds, dbias = torch.full((32, 4), 3.0, device="cuda"), torch.full((2, 64), 3.0, device="cuda")
    dy2, s, bias = torch.randn(32, 64, device="cuda"), torch.rand(32, 4, device="cuda"), torch.randn(2, 64, device="cuda")
    assert L.lib.bist_scaled_bias_bwd_det(dy2.data_ptr(), s.data_ptr(), bias.data_ptr(), ds.data_ptr(), dbias.data_ptr(), 32, 4, 16, 2, 64, 64,
                                          _code(torch.float32), ws.data_ptr(), need - 4, _stream()) != 0
    torch.cuda.synchronize()
    for t in (out, da, db, ds, dbias):
        assert (t == 3.0).all()
