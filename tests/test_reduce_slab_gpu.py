"""The slab reductions of reduce_slab.hip at the C ABI: column sums (bias gradients) and LayerNorm gain / offset gradients, one launch
per batch of jobs, one atomic per destination element per job.

Accuracy bounds are those of tests/test_det_reduce_gpu.py: the worst case of ANY fp32 summation order, n * 2^-23 * sum|terms| against an
fp64 sum of the same (already rounded) inputs, per output element; the LayerNorm terms are formed as that file forms them.  A
destination that already holds a value is one more term of its element's sum.  The protocol tests ask for bit equality: with pairwise
disjoint destinations every element receives exactly one add of a total that is summed in chunk order."""
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23
DTYPES = [torch.float32, torch.bfloat16]
HEADER = 256


def _lib():
    from bist_amd import _lib
    return _lib


def _code(dt):
    from bist_amd.ops import dtype_code
    return dtype_code(dt)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _wide(shape, gen, lo=-3.0, hi=3.0):
    """randn * 10^U(lo, hi): magnitudes over several decades, so that the order of an fp32 sum shows in its bits."""
    return torch.randn(shape, generator=gen, device="cuda") * 10.0 ** (torch.rand(shape, generator=gen, device="cuda") * (hi - lo) + lo)


def _workspace(nbytes):
    ws = torch.empty(max(nbytes, HEADER) // 4, device="cuda", dtype=torch.float32)
    ws[:HEADER // 4].zero_()
    return ws


# ---- column sums ---------------------------------------------------------------------------------------------------------------------
def _col_arr(xs, outs):
    L = _lib()
    arr = (L.BistColSum * len(xs))()
    for i, (x, o) in enumerate(zip(xs, outs)):
        arr[i].x, arr[i].out, arr[i].M, arr[i].N, arr[i].ldx = x.data_ptr(), o.data_ptr(), x.shape[0], x.shape[1], x.stride(0)
    return arr


def _col_sum(xs, outs, ws=None, ws_bytes=None):
    L = _lib()
    arr = _col_arr(xs, outs)
    need = L.lib.bist_col_sum_multi_ws_workspace(arr, len(xs))
    assert need > HEADER
    if ws is None:
        ws = _workspace(need)
    rc = L.lib.bist_col_sum_multi_ws(arr, len(xs), _code(xs[0].dtype), ws.data_ptr(), ws.numel() * 4 if ws_bytes is None else ws_bytes, _stream())
    return rc, need


def _col_check(x, out, out0=None):
    """|out - fp64 sum| <= n * 2^-23 * sum|terms| per column; out0: what the destination held before (one more term)."""
    M = x.shape[0]
    ref, mag, n = x.double().sum(0), x.double().abs().sum(0), M
    if out0 is not None:
        ref, mag, n = ref + out0.double(), mag + out0.double().abs(), M + 1
    err, bound = (out.double() - ref).abs(), n * EPS32 * mag
    assert (err <= bound).all(), (tuple(x.shape), x.dtype, (err / bound.clamp_min(1e-300)).max().item())
    return (err / bound.clamp_min(1e-300)).max().item()


# one chunk, the chunk edge, a short last chunk, three chunks with a one-row tail, a chunk size above the minimum (17 rows) x
# one 16-byte piece, a quarter block, past the 512-column workgroup
COL_SPECS = [(M, N) for M in (1, 16, 17, 33, 2049) for N in (8, 64, 520)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_col_sums_meet_the_fp32_bound_alone_and_accumulate(dtype):
    g = _gen(1)
    specs = COL_SPECS + ([(33, 7)] if dtype == torch.float32 else [])          # N = 7: the scalar path
    worst = 0.0
    for M, N in specs:
        x = _wide((M, N), g).to(dtype)
        out = torch.zeros(N, device="cuda")
        rc, _ = _col_sum([x], [out])
        assert rc == 0, _lib().lib.bist_last_error()
        worst = max(worst, _col_check(x, out))
        out0 = torch.randn(N, generator=g, device="cuda")
        out = out0.clone()
        rc, _ = _col_sum([x], [out])
        assert rc == 0, _lib().lib.bist_last_error()
        worst = max(worst, _col_check(x, out, out0))
    print("col sums %s: max err / bound %.3f over %d shapes" % (dtype, worst, len(specs)))


def test_col_sum_scalar_path_on_an_unaligned_leading_dimension():
    g = _gen(2)
    big = _wide((45, 21), g)
    x = big[:, 3:10]                                 # N = 7, ld = 21, base 12 bytes into a row
    out = torch.zeros(7, device="cuda")
    rc, _ = _col_sum([x], [out])
    assert rc == 0, _lib().lib.bist_last_error()
    _col_check(x, out)


# ---- LayerNorm gain / offset gradients ----------------------------------------------------------------------------------------------
def _ln_inputs(rows, d, dtype, seed):
    g = _gen(seed)
    x = (torch.randn((rows, d), generator=g, device="cuda") * 2.0 + 0.5).to(dtype)
    dy = _wide((rows, d), g, -1.0, 1.0).to(dtype)
    a = torch.ones(d, device="cuda", dtype=dtype)
    return dy, x, a


def _ln_arr(jobs, eps):
    L = _lib()
    arr = (L.BistLnGrad * len(jobs))()
    for i, (dy, x, a, da, db) in enumerate(jobs):
        arr[i].dy, arr[i].x, arr[i].a, arr[i].da, arr[i].db = dy.data_ptr(), x.data_ptr(), a.data_ptr(), da.data_ptr(), db.data_ptr()
        arr[i].rows, arr[i].lddy, arr[i].ldx, arr[i].eps = x.shape[0], dy.stride(0), x.stride(0), eps
    return arr


def _ln_grad(jobs, d, eps=1e-6, ws=None, ws_bytes=None):
    """jobs: (dy, x, a, da, db)"""
    L = _lib()
    arr = _ln_arr(jobs, eps)
    need = L.lib.bist_layernorm_param_grad_multi_ws_workspace(arr, len(jobs), d)
    assert need > HEADER
    if ws is None:
        ws = _workspace(need)
    return L.lib.bist_layernorm_param_grad_multi_ws(arr, len(jobs), d, _code(jobs[0][0].dtype), ws.data_ptr(),
                                                    ws.numel() * 4 if ws_bytes is None else ws_bytes, _stream())


def _ln_check(dy, x, da, db, eps=1e-6):
    rows = x.shape[0]
    xd, gd = x.double(), dy.double()
    xc = xd - xd.mean(1, keepdim=True)
    term = gd * xc / (xd.std(1, keepdim=True) + eps)          # unbiased std, eps outside the root (modules.py:28-31)
    ea, eb = (da.double() - term.sum(0)).abs(), (db.double() - gd.sum(0)).abs()
    ba, bb = rows * EPS32 * term.abs().sum(0), rows * EPS32 * gd.abs().sum(0)
    ra, rb = (ea / ba.clamp_min(1e-300)).max().item(), (eb / bb.clamp_min(1e-300)).max().item()
    print("ln grads %s [%d x %d]: max err / bound da %.3f db %.3f" % (x.dtype, rows, x.shape[1], ra, rb))
    assert (ea <= ba).all() and (eb <= bb).all(), (rows, ra, rb)


# one row, one trip of a wave, a trip and a row, three chunks with a short last one, a one-row last chunk
@pytest.mark.parametrize("dtype,d", [(torch.bfloat16, 512), (torch.float32, 256)], ids=["bf16-512", "f32-256"])
@pytest.mark.parametrize("rows", [1, 4, 5, 37, 321])
def test_layernorm_param_grads_meet_the_fp32_bound(rows, dtype, d):
    dy, x, a = _ln_inputs(rows, d, dtype, 3 + rows)
    da, db = torch.zeros(d, device="cuda"), torch.zeros(d, device="cuda")
    assert _ln_grad([(dy, x, a, da, db)], d) == 0, _lib().lib.bist_last_error()
    _ln_check(dy, x, da, db)


# ---- batching ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_49_column_sum_jobs_and_a_shared_destination(dtype):
    """49 jobs: one more than a launch takes.  Jobs 5 and 48 (second launch) add into ONE destination."""
    g = _gen(4)
    specs = [(1 + (37 * i) % 300, 8 * (1 + (5 * i) % 70)) for i in range(49)]
    specs[48] = (77, specs[5][1])
    xs = [_wide(s, g).to(dtype) for s in specs]
    outs = [torch.zeros(s[1], device="cuda") for s in specs]
    outs[48] = outs[5]
    rc, _ = _col_sum(xs, outs)
    assert rc == 0, _lib().lib.bist_last_error()
    torch.cuda.synchronize()
    for i, (x, o) in enumerate(zip(xs, outs)):
        if i not in (5, 48):
            _col_check(x, o)
    _col_check(torch.cat([xs[5], xs[48]]), outs[5])           # the sum of both jobs


@pytest.mark.parametrize("dtype,d", [(torch.bfloat16, 512), (torch.float32, 256)], ids=["bf16-512", "f32-256"])
def test_41_layernorm_jobs_and_a_shared_destination(dtype, d):
    jobs = []
    for i in range(41):
        dy, x, a = _ln_inputs(1 + (53 * i) % 200, d, dtype, 100 + i)
        jobs.append((dy, x, a, torch.zeros(d, device="cuda"), torch.zeros(d, device="cuda")))
    jobs[40] = jobs[40][:3] + jobs[7][3:]                      # job 40 (second launch) shares job 7's destinations
    assert _ln_grad(jobs, d) == 0, _lib().lib.bist_last_error()
    torch.cuda.synchronize()
    for i, (dy, x, a, da, db) in enumerate(jobs):
        if i not in (7, 40):
            _ln_check(dy, x, da, db)
    _ln_check(torch.cat([jobs[7][0], jobs[40][0]]), torch.cat([jobs[7][1], jobs[40][1]]), jobs[7][3], jobs[7][4])


# ---- protocol -------------------------------------------------------------------------------------------------------------------------
def _protocol_case():
    g = _gen(6)
    specs = [(2049, 520), (333, 64), (17, 8), (1, 520), (700, 512)]
    xs = [_wide(s, g).to(torch.bfloat16) for s in specs]
    base = [torch.randn(s[1], generator=g, device="cuda") for s in specs]
    ln = [_ln_inputs(r, 512, torch.bfloat16, 50 + r) for r in (321, 37, 5)]
    lbase = [(torch.randn(512, generator=g, device="cuda"), torch.randn(512, generator=g, device="cuda")) for _ in ln]
    L = _lib()
    need = max(L.lib.bist_col_sum_multi_ws_workspace(_col_arr(xs, base), len(xs)),
               L.lib.bist_layernorm_param_grad_multi_ws_workspace(_ln_arr([(dy, x, a, p, q) for (dy, x, a), (p, q) in zip(ln, lbase)], 1e-6), len(ln), 512))
    return xs, base, ln, lbase, _workspace(need)


def test_back_to_back_calls_and_graph_replays_give_the_same_bits():
    """ONE workspace, the same two calls over and over: a counter that does not return to zero, or a slab read before it is visible,
    changes the bits of a later run."""
    from bist_amd import functional as Fn
    xs, base, ln, lbase, ws = _protocol_case()
    outs = [b.clone() for b in base]
    louts = [(p.clone(), q.clone()) for p, q in lbase]

    def reset():
        for o, b in zip(outs, base):
            o.copy_(b)
        for (p, q), (p0, q0) in zip(louts, lbase):
            p.copy_(p0)
            q.copy_(q0)

    def call():
        rc, _ = _col_sum(xs, outs, ws=ws)
        assert rc == 0, _lib().lib.bist_last_error()
        assert _ln_grad([(dy, x, a, p, q) for (dy, x, a), (p, q) in zip(ln, louts)], 512, ws=ws) == 0, _lib().lib.bist_last_error()

    def snapshot():
        torch.cuda.synchronize()
        return [o.clone() for o in outs] + [t.clone() for pq in louts for t in pq]
    runs = []
    for _ in range(3):                                  # three calls back to back, no host synchronisation inside a run
        reset()
        call()
        runs.append(snapshot())
    for x, o, b in zip(xs, runs[0], base):
        _col_check(x, o, b)
    graph = Fn.Graph()
    with Fn.capture_graph(graph):
        call()
    for _ in range(3):
        reset()
        graph.replay()
        runs.append(snapshot())
    assert (ws[:HEADER // 4].view(torch.int32) == 0).all()      # every counter is back at zero
    for k, r in enumerate(runs[1:], 1):
        for a, b in zip(runs[0], r):
            assert torch.equal(a, b), "run %d differs from run 0" % k


def test_an_undersized_workspace_is_refused_and_nothing_is_launched():
    L = _lib()
    x = _wide((200, 96), _gen(11))
    out = torch.full((96,), 3.0, device="cuda")
    ws = _workspace(1 << 18)
    rc, need = _col_sum([x], [out], ws=ws, ws_bytes=0)
    assert need == HEADER + 13 * 96 * 4                  # 200 rows in chunks of 16
    assert rc != 0
    rc, _ = _col_sum([x], [out], ws=ws, ws_bytes=need - 4)
    assert rc != 0 and b"workspace" in L.lib.bist_last_error()
    dy, xx, a = _ln_inputs(37, 256, torch.float32, 12)
    da, db = torch.full((256,), 3.0, device="cuda"), torch.full((256,), 3.0, device="cuda")
    arr = _ln_arr([(dy, xx, a, da, db)], 1e-6)
    need = L.lib.bist_layernorm_param_grad_multi_ws_workspace(arr, 1, 256)
    assert need == HEADER + 3 * 2 * 256 * 4              # 37 rows in chunks of 16
    assert _ln_grad([(dy, xx, a, da, db)], 256, ws=ws, ws_bytes=need - 4) != 0
    assert b"workspace" in L.lib.bist_last_error()
    torch.cuda.synchronize()
    for t in (out, da, db):
        assert (t == 3.0).all()
    assert (ws[:HEADER // 4].view(torch.int32) == 0).all()
