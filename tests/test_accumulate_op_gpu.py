"""bist_adam_accum_dev alone: the accumulating phases, the closing phase against bist_adam_step_dev on the fp32
sum, a group of one against bist_adam_step_dev_bg, and the refused calls.  Sizes: the smallest vector case, a partial last workgroup,
several grid-stride trips with a remainder (background form), and the scalar form (n % 4 != 0, pointers off by one element).  Every
comparison is torch.equal; every buffer carries guard elements behind its range that must stay as they were."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B1, B2, EPS = 0.9, 0.98, 1e-9
GUARD = 8
EINVAL = -1                                                       # BIST_EINVAL (include/bist_hip.h)
# (n, max_blocks, pointer offset in elements)
CASES = [(8, 0, 0), (2052, 0, 0), (5132, 2, 0), (1027, 0, 0), (1027, 0, 1), (1028, 0, 1)]
IDS = ["n8", "n2052", "n5132-bg2", "n1027", "n1027-off1", "n1028-off1"]
GDT = {"gbf16": torch.bfloat16, "gf32": torch.float32}
WDT = {"nowork": None, "wbf16": torch.bfloat16}


def _lib():
    from bist_amd import _lib as L
    return L


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _code(dt):
    return 1 if dt == torch.bfloat16 else 0


class _State:
    """p, m, v (f32), work (bf16 or None), acc (f32, NaN), the scalars: each tensor off + n + GUARD elements, the range at [off, off + n)."""

    def __init__(self, n, off, wdt, seed=5):
        g = torch.Generator(device="cuda").manual_seed(seed)
        N = off + n + GUARD
        self.n, self.off = n, off
        self.p = torch.randn(N, device="cuda", generator=g)
        self.m = 0.1 * torch.randn(N, device="cuda", generator=g)
        self.v = 0.01 * torch.rand(N, device="cuda", generator=g)
        self.work = torch.full((N,), 7.0, device="cuda", dtype=wdt) if wdt is not None else None
        self.acc = torch.full((N,), float("nan"), device="cuda")
        # {lr, 1 - b1^t, 1 - b2^t, grad_scale} of step t = 3, a grad_scale that is no power of two
        self.hyper = torch.tensor([1e-2, 1 - B1 ** 3, 1 - B2 ** 3, 0.37, 1.0, 0, 0, 0], device="cuda", dtype=torch.float32)
        self.phase = torch.zeros(1, device="cuda", dtype=torch.int32)

    def clone(self):
        c = object.__new__(_State)
        c.__dict__.update({k: (x.clone() if isinstance(x, torch.Tensor) else x) for k, x in self.__dict__.items()})
        return c

    def ptr(self, t):
        return None if t is None else t.data_ptr() + self.off * t.element_size()

    def bufs(self):
        return {"p": self.p, "m": self.m, "v": self.v, "work": self.work, "acc": self.acc}


def _grad(n, off, dt, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(off + n + GUARD, device="cuda", generator=g).to(dt)


def _accum(s, g, phase, max_blocks=0, acc=True, ph=True):
    s.phase.fill_(phase)
    return _lib().lib.bist_adam_accum_dev(s.ptr(s.p), s.ptr(g), s.ptr(s.acc) if acc else None, s.ptr(s.m), s.ptr(s.v), s.ptr(s.work), s.n,
                                         s.hyper.data_ptr(), s.phase.data_ptr() if ph else None, B1, B2, EPS, _code(g.dtype),
                                         _code(s.work.dtype) if s.work is not None else 0, max_blocks, _stream())


def _adam(s, g, max_blocks=None):
    L = _lib().lib
    args = (s.ptr(s.p), s.ptr(g), s.ptr(s.m), s.ptr(s.v), s.ptr(s.work), s.n, s.hyper.data_ptr(), B1, B2, EPS, _code(g.dtype),
            _code(s.work.dtype) if s.work is not None else 0)
    if max_blocks is None:
        return L.bist_adam_step_dev(*args, _stream())
    return L.bist_adam_step_dev_bg(*args, max_blocks, _stream())


def _equal(a, b, names, what):
    for k in names:
        x, y = a.bufs()[k], b.bufs()[k]
        if x is None:
            assert y is None
            continue
        # (NaN-filled accumulators compare by their bits)
        same = torch.equal(x.view(torch.int32), y.view(torch.int32)) if x.dtype == torch.float32 else torch.equal(x.view(torch.int16), y.view(torch.int16))
        assert same, "%s: %s differs" % (what, k)


@pytest.mark.parametrize("wname", list(WDT))
@pytest.mark.parametrize("gname", list(GDT))
@pytest.mark.parametrize("n,max_blocks,off", CASES, ids=IDS)
def test_phases_accumulate_in_fp32_and_close_with_adam_on_the_sum(n, max_blocks, off, gname, wname):
    gdt, wdt = GDT[gname], WDT[wname]
    s0 = _State(n, off, wdt)
    g1, g2, g3 = (_grad(n, off, gdt, seed) for seed in (11, 12, 13))
    keep = [g.clone() for g in (g1, g2, g3)]
    lo, hi = off, off + n
    s = s0.clone()
    # first pass: acc = float(g1), read from a NaN-filled accumulator
    assert _accum(s, g1, 1, max_blocks) == 0, _lib().lib.bist_last_error()
    a = g1.float().clone()                                       # (.float() of an fp32 gradient is the gradient itself)
    assert torch.equal(s.acc[lo:hi], a[lo:hi])
    assert torch.isnan(s.acc[:lo]).all() and torch.isnan(s.acc[hi:]).all()
    _equal(s, s0, ("p", "m", "v", "work"), "after phase 1")
    # middle pass: acc += float(g2), one fp32 add
    assert _accum(s, g2, 0, max_blocks) == 0, _lib().lib.bist_last_error()
    a += g2.float()
    assert torch.equal(s.acc[lo:hi], a[lo:hi])
    assert torch.isnan(s.acc[:lo]).all() and torch.isnan(s.acc[hi:]).all()
    _equal(s, s0, ("p", "m", "v", "work"), "after phase 0")
    # last pass: Adam on acc + float(g3), against bist_adam_step_dev fed that sum in fp32 from the same starting state
    before = s.clone()
    assert _accum(s, g3, 2, max_blocks) == 0, _lib().lib.bist_last_error()
    ref = s0.clone()
    total = a + g3.float()
    assert _adam(ref, total) == 0, _lib().lib.bist_last_error()
    torch.cuda.synchronize()
    _equal(s, ref, ("p", "m", "v", "work"), "after phase 2")
    assert not torch.equal(s.p[lo:hi], s0.p[lo:hi])
    _equal(s, before, ("acc",), "phase 2 wrote the accumulator")
    for k in ("p", "m", "v", "work"):                            # the guard elements on both sides of the range
        x, y = s.bufs()[k], s0.bufs()[k]
        if x is not None:
            assert torch.equal(x[:lo], y[:lo]) and torch.equal(x[hi:], y[hi:]), k
    for g, k in zip((g1, g2, g3), keep):
        assert torch.equal(g, k), "a gradient was written"


@pytest.mark.parametrize("wname", list(WDT))
@pytest.mark.parametrize("gname", list(GDT))
@pytest.mark.parametrize("n,max_blocks,off", CASES, ids=IDS)
def test_a_group_of_one_is_the_plain_update(n, max_blocks, off, gname, wname):
    gdt, wdt = GDT[gname], WDT[wname]
    s0 = _State(n, off, wdt)
    g1 = _grad(n, off, gdt, 11)
    s, ref = s0.clone(), s0.clone()
    assert _accum(s, g1, 3, max_blocks) == 0, _lib().lib.bist_last_error()
    assert _adam(ref, g1, max_blocks) == 0, _lib().lib.bist_last_error()
    torch.cuda.synchronize()
    _equal(s, ref, ("p", "m", "v", "work"), "phase 3")
    _equal(s, s0, ("acc",), "phase 3 wrote the accumulator")
    assert not torch.equal(s.p[off:off + n], s0.p[off:off + n])


def test_bad_calls_are_refused_before_any_launch():
    L = _lib().lib
    s0 = _State(1028, 0, torch.bfloat16)
    g = _grad(1028, 0, torch.bfloat16, 11)
    s = s0.clone()
    assert _accum(s, g, 3, acc=False) == EINVAL and b"bist_adam_accum_dev" in L.bist_last_error()
    assert _accum(s, g, 3, ph=False) == EINVAL and b"bist_adam_accum_dev" in L.bist_last_error()
    s.n = 1027                                                    # the background form on a range that is no whole 16-byte groups
    assert _accum(s, g, 3, max_blocks=2) == EINVAL and b"background" in L.bist_last_error()
    s.n, s.off = 1024, 1                                          # ... and on misaligned pointers
    assert _accum(s, g, 3, max_blocks=2) == EINVAL and b"background" in L.bist_last_error()
    torch.cuda.synchronize()
    _equal(s, s0, ("p", "m", "v", "work", "acc"), "a refused call")
