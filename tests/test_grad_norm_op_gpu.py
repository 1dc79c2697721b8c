"""bist_grad_sumsq, bist_clip_hyper and the guarded Adam launches alone, through the C ABI.

Sum of squares: lengths 1, 3, 8, 255, 1 029 and 2^20 + 7 (one element, less than a 16-byte line, exactly one bf16 line, less than a
workgroup's first trip, a remainder behind whole lines, many trips with a remainder), 1 / 7 / 64 slots (so also more slots than
elements: empty slots), bf16 and fp32, the base pointer 0, 1 and 3 elements into a larger buffer (scalar head and tail).  The
reference sums the same bf16 / fp32 values in float64 with torch, so only the order of fp64 additions differs: relative 1e-12."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B1, B2, EPS = 0.9, 0.98, 1e-9
EINVAL = -1                                                       # BIST_EINVAL (include/bist_hip.h)
LENGTHS = [1, 3, 8, 255, 1029, 2 ** 20 + 7]
NSLOTS = [1, 7, 64]
OFFSETS = [0, 1, 3]
DT = {"bf16": torch.bfloat16, "f32": torch.float32}
PAD = 16                                                          # elements behind every range


def _L():
    from bist_amd import _lib
    return _lib.lib


def _err():
    return _L().bist_last_error()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _code(dt):
    return 1 if dt == torch.bfloat16 else 0


def _chunk(n, nslots):
    return ((n + nslots - 1) // nslots + 7) // 8 * 8


def _data(n, dt, seed=3):
    """3 + n + PAD elements; the range of offset `off` is [off, off + n)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(3 + n + PAD, device="cuda", generator=g).to(dt)


def _sumsq(buf, off, n, nslots, slab=None, slot_lo=0, max_blocks=0, acc=None, phase=None):
    """Launch over buf[off: off + n] into a NaN-poisoned slab of slot_lo + nslots + 2 slots (or the slab given); returns the slab."""
    if slab is None:
        slab = torch.full((slot_lo + nslots + 2,), float("nan"), device="cuda", dtype=torch.float64)
    rc = _L().bist_grad_sumsq(buf.data_ptr() + off * buf.element_size(), None if acc is None else acc.data_ptr() + 4 * off,
                              None if phase is None else phase.data_ptr(), n, _code(buf.dtype), slab.data_ptr(), slot_lo, nslots,
                              max_blocks, _stream())
    assert rc == 0, _err()
    return slab


def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


# ---- 1. against torch in float64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", list(DT))
@pytest.mark.parametrize("n", LENGTHS)
def test_sum_of_squares_against_float64(n, dname):
    buf = _data(n, DT[dname])
    for off in OFFSETS:
        x = buf[off:off + n].double()
        want = (x * x).sum().item()
        for nslots in NSLOTS:
            slab = _sumsq(buf, off, n, nslots, slot_lo=1)
            torch.cuda.synchronize()
            assert torch.isnan(slab[0]) and torch.isnan(slab[1 + nslots:]).all(), "a slot outside the range was written"
            part = slab[1:1 + nslots]
            assert not torch.isnan(part).any(), "a slot of the range was not written"
            got = part.sum().item()
            print("n %d off %d nslots %d: %.17g vs %.17g rel %.3g" % (n, off, nslots, got, want, abs(got - want) / want))
            assert abs(got - want) <= 1e-12 * want, (n, off, nslots, got, want)
            ch = _chunk(n, nslots)
            for s in range(nslots):                               # every slot is its own chunk; an empty chunk reads back as exactly 0.0
                c = x[s * ch: (s + 1) * ch]
                if c.numel() == 0:
                    assert part[s].item() == 0.0 and not math.copysign(1.0, part[s].item()) < 0, (n, nslots, s)
                else:
                    w = (c * c).sum().item()
                    assert abs(part[s].item() - w) <= 1e-12 * w, (n, off, nslots, s)


# ---- 2. the slots' bits depend on (data, n, nslots) alone ----------------------------------------------------------------------------
@pytest.mark.parametrize("dname", list(DT))
@pytest.mark.parametrize("n,nslots", [(1029, 7), (2 ** 20 + 7, 7), (2 ** 20 + 7, 64), (3, 64)])
def test_slots_are_bit_equal_across_launches_and_grids(n, nslots, dname):
    buf = _data(n, DT[dname])
    first = _sumsq(buf, 1, n, nslots)
    for max_blocks in (0, 0, 1, 3):
        again = _sumsq(buf, 1, n, nslots, max_blocks=max_blocks)
        torch.cuda.synchronize()
        assert torch.equal(_bits(first), _bits(again)), "max_blocks %d" % max_blocks


# ---- 3. the accumulating forms ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", list(DT))
@pytest.mark.parametrize("n,off", [(1029, 0), (1029, 1), (2 ** 20 + 7, 0), (8, 3)])
def test_acc_and_phase_forms(n, off, dname):
    nslots = 7
    buf = _data(n, DT[dname])
    acc = _data(n, torch.float32, seed=4)
    phase = torch.zeros(1, device="cuda", dtype=torch.int32)
    poison = torch.full((nslots + 2,), float("nan"), device="cuda", dtype=torch.float64)
    for ph in (0, 1):                                             # not the last pass: nothing is stored
        phase.fill_(ph)
        slab = _sumsq(buf, off, n, nslots, acc=acc, phase=phase)
        torch.cuda.synchronize()
        assert torch.equal(_bits(slab), _bits(poison)), "phase %d wrote the slab" % ph
    g = buf[off:off + n]
    # a group of one: the gradient alone, the accumulator (NaN) is not read into the result; the bits of the launch without acc
    phase.fill_(3)
    slab = _sumsq(buf, off, n, nslots, acc=torch.full_like(acc, float("nan")), phase=phase)
    plain = _sumsq(buf, off, n, nslots)
    torch.cuda.synchronize()
    assert torch.equal(_bits(slab), _bits(plain))
    # the last pass of a longer group: float32(acc + g), squared in fp64
    phase.fill_(2)
    slab = _sumsq(buf, off, n, nslots, acc=acc, phase=phase)
    s = (acc[off:off + n] + g.float()).double()
    want = (s * s).sum().item()
    got = slab[:nslots].sum().item()
    assert abs(got - want) <= 1e-12 * want, (got, want)
    assert torch.isnan(slab[nslots:]).all()


# ---- 4. bist_clip_hyper ---------------------------------------------------------------------------------------------------------------
NS_TOTAL = 71                                                    # two ranges: 64 + 7 slots


def _hyper(gscale=0.37):
    return torch.tensor([1e-2, 0.271, 0.0588, gscale, 1.0, 7.0, 7.0, 7.0], device="cuda", dtype=torch.float32)


def _clip(part, max_norm, hyper, ctr, phase=None):
    return _L().bist_clip_hyper(part.data_ptr(), part.numel(), max_norm, hyper.data_ptr(), ctr.data_ptr(),
                                None if phase is None else phase.data_ptr(), _stream())


def _partials():
    g = torch.Generator(device="cuda").manual_seed(9)
    return torch.rand(NS_TOTAL, device="cuda", generator=g, dtype=torch.float64) * 3.0 + 0.01


def test_clip_hyper_writes_norm_scale_and_grad_scale():
    part = _partials()
    gs = np.float32(0.37)
    norm64 = math.sqrt(part.sum().item()) * float(gs)
    ctr = torch.zeros(1, device="cuda", dtype=torch.int64)
    for max_norm in (0.5 * norm64, 2.0 * norm64, 1e-3):
        h = _hyper()
        assert _clip(part, max_norm, h, ctr) == 0, _err()
        out = h.cpu().numpy()
        assert abs(float(out[6]) - norm64) <= 1e-6 * norm64, (out[6], norm64)
        scale = np.minimum(np.float32(1.0), np.float32(max_norm) / (out[6] + np.float32(1e-6)))
        assert scale.dtype == np.float32 and out[7] == scale, (out[7], scale)
        assert out[3] == gs * scale and out[5] == 0.0
        assert (scale < 1) == (max_norm < norm64)
        assert np.array_equal(out[:3], _hyper().cpu().numpy()[:3]) and out[4] == 1.0
    assert int(ctr) == 0


@pytest.mark.parametrize("gscale", [0.37, 1.0])
def test_clip_hyper_with_an_infinite_bound_leaves_grad_scale_bit_for_bit(gscale):
    part = _partials()
    ctr = torch.zeros(1, device="cuda", dtype=torch.int64)
    h = _hyper(gscale)
    assert _clip(part, math.inf, h, ctr) == 0, _err()
    assert torch.equal(_bits(h[3:4]), _bits(_hyper(gscale)[3:4])) and h[7].item() == 1.0 and h[5].item() == 0.0
    assert h[6].item() > 0 and int(ctr) == 0


def test_clip_hyper_skips_a_non_finite_norm_and_counts_it():
    ctr = torch.full((1,), 5, device="cuda", dtype=torch.int64)
    good = _partials()
    for k, bad in enumerate((float("inf"), float("nan"))):
        part = good.clone()
        part[40] = bad
        h = _hyper()
        assert _clip(part, 1.0, h, ctr) == 0, _err()
        assert h[5].item() == 1.0 and h[7].item() == 0.0 and not math.isfinite(h[6].item())
        assert torch.equal(_bits(h[3:4]), _bits(_hyper()[3:4])), "grad_scale changed on a skipped step"
        assert int(ctr) == 6 + k
        # a finite case afterwards resets the skip word and leaves the counter alone
        assert _clip(good, 1.0, h, ctr) == 0, _err()
        assert h[5].item() == 0.0 and h[7].item() > 0 and int(ctr) == 6 + k


def test_clip_hyper_outside_the_last_pass_only_clears_the_skip_word():
    part = torch.full((NS_TOTAL,), float("nan"), device="cuda", dtype=torch.float64)      # never read
    ctr = torch.zeros(1, device="cuda", dtype=torch.int64)
    phase = torch.zeros(1, device="cuda", dtype=torch.int32)
    for ph in (0, 1):
        phase.fill_(ph)
        h = _hyper()
        assert _clip(part, 1.0, h, ctr, phase) == 0, _err()
        want = _hyper()
        want[5] = 0.0
        assert torch.equal(_bits(h), _bits(want)) and int(ctr) == 0
    phase.fill_(2)
    h = _hyper()
    assert _clip(_partials(), 1.0, h, ctr, phase) == 0, _err()
    assert h[6].item() > 0 and h[7].item() > 0 and h[5].item() == 0.0


# ---- 5. guarded Adam ------------------------------------------------------------------------------------------------------------------
class _State:
    def __init__(self, n, wdt, seed=5):
        g = torch.Generator(device="cuda").manual_seed(seed)
        N = n + PAD
        self.n = n
        self.p = torch.randn(N, device="cuda", generator=g)
        self.m = 0.1 * torch.randn(N, device="cuda", generator=g)
        self.v = 0.01 * torch.rand(N, device="cuda", generator=g)
        self.work = torch.full((N,), 7.0, device="cuda", dtype=wdt) if wdt is not None else None
        self.acc = 0.5 * torch.randn(N, device="cuda", generator=g)
        self.hyper = torch.tensor([1e-2, 1 - B1 ** 3, 1 - B2 ** 3, 0.37, 1.0, 0, 0, 0], device="cuda", dtype=torch.float32)
        self.phase = torch.zeros(1, device="cuda", dtype=torch.int32)

    def clone(self):
        c = object.__new__(_State)
        c.__dict__.update({k: (x.clone() if isinstance(x, torch.Tensor) else x) for k, x in self.__dict__.items()})
        return c

    def bufs(self):
        return {"p": self.p, "m": self.m, "v": self.v, "work": self.work, "acc": self.acc}


def _ptr(t):
    return None if t is None else t.data_ptr()


def _step(s, g, guard, max_blocks):
    fn = _L().bist_adam_step_dev_guard if guard else _L().bist_adam_step_dev_bg
    rc = fn(_ptr(s.p), _ptr(g), _ptr(s.m), _ptr(s.v), _ptr(s.work), s.n, s.hyper.data_ptr(), B1, B2, EPS, _code(g.dtype),
            _code(s.work.dtype) if s.work is not None else 0, max_blocks, _stream())
    assert rc == 0, _err()


def _accum(s, g, guard, max_blocks, phase):
    s.phase.fill_(phase)
    fn = _L().bist_adam_accum_dev_guard if guard else _L().bist_adam_accum_dev
    rc = fn(_ptr(s.p), _ptr(g), _ptr(s.acc), _ptr(s.m), _ptr(s.v), _ptr(s.work), s.n, s.hyper.data_ptr(), s.phase.data_ptr(), B1, B2, EPS,
            _code(g.dtype), _code(s.work.dtype) if s.work is not None else 0, max_blocks, _stream())
    assert rc == 0, _err()


def _same(a, b, names, what):
    for k in names:
        x, y = a.bufs()[k], b.bufs()[k]
        if x is None:
            assert y is None
            continue
        assert torch.equal(_bits(x), _bits(y)), "%s: %s differs" % (what, k)


ADAM_CASES = [(1029, 0), (4096, 0), (4096, 2)]                   # scalar kernel, vector kernel, vector kernel as a background launch


@pytest.mark.parametrize("gname,wdt", [("bf16", torch.bfloat16), ("f32", None)], ids=["bf16", "f32"])
@pytest.mark.parametrize("n,max_blocks", ADAM_CASES, ids=["n1029", "n4096", "n4096-bg2"])
def test_guarded_step_is_the_plain_step_or_nothing(n, max_blocks, gname, wdt):
    s0 = _State(n, wdt)
    g = _data(n, DT[gname], seed=11)[:n + PAD]
    plain, open_ = s0.clone(), s0.clone()
    _step(plain, g, False, max_blocks)
    _step(open_, g, True, max_blocks)
    torch.cuda.synchronize()
    assert not torch.equal(plain.p[:n], s0.p[:n])
    _same(open_, plain, ("p", "m", "v", "work"), "hyper[5] = 0")
    shut = s0.clone()
    shut.hyper[5] = 1.0
    _step(shut, g, True, max_blocks)
    torch.cuda.synchronize()
    _same(shut, s0, ("p", "m", "v", "work"), "hyper[5] = 1")


@pytest.mark.parametrize("gname,wdt", [("bf16", torch.bfloat16), ("f32", None)], ids=["bf16", "f32"])
@pytest.mark.parametrize("n,max_blocks", ADAM_CASES, ids=["n1029", "n4096", "n4096-bg2"])
def test_guarded_accumulating_step_guards_the_last_pass_only(n, max_blocks, gname, wdt):
    s0 = _State(n, wdt)
    g = _data(n, DT[gname], seed=11)[:n + PAD]
    for phase in (3, 2):                                          # the passes that run Adam
        plain, open_ = s0.clone(), s0.clone()
        _accum(plain, g, False, max_blocks, phase)
        _accum(open_, g, True, max_blocks, phase)
        torch.cuda.synchronize()
        assert not torch.equal(plain.p[:n], s0.p[:n])
        _same(open_, plain, ("p", "m", "v", "work", "acc"), "phase %d, hyper[5] = 0" % phase)
        shut = s0.clone()
        shut.hyper[5] = 1.0
        _accum(shut, g, True, max_blocks, phase)
        torch.cuda.synchronize()
        _same(shut, s0, ("p", "m", "v", "work", "acc"), "phase %d, hyper[5] = 1" % phase)
    for phase in (1, 0):                                          # first and middle passes accumulate whatever the skip word says
        plain, shut = s0.clone(), s0.clone()
        shut.hyper[5] = 1.0
        _accum(plain, g, False, max_blocks, phase)
        _accum(shut, g, True, max_blocks, phase)
        torch.cuda.synchronize()
        assert not torch.equal(plain.acc[:n], s0.acc[:n])
        _same(shut, plain, ("p", "m", "v", "work", "acc"), "phase %d, hyper[5] = 1" % phase)
        _same(shut, s0, ("p", "m", "v", "work"), "phase %d wrote the weights" % phase)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def test_bad_calls_are_refused_before_any_launch():
    from bist_amd import _lib
    L = _L()
    buf = _data(64, torch.bfloat16)
    acc = _data(64, torch.float32)
    phase = torch.zeros(1, device="cuda", dtype=torch.int32)
    slab = torch.full((8,), float("nan"), device="cuda", dtype=torch.float64)
    st = _stream()

    def sumsq(g=buf.data_ptr(), a=None, ph=None, n=64, part=slab.data_ptr(), slot_lo=0, nslots=4):
        return L.bist_grad_sumsq(g, a, ph, n, 1, part, slot_lo, nslots, 0, st)
    assert sumsq(g=None) == EINVAL and b"bist_grad_sumsq" in _err()
    assert sumsq(part=None) == EINVAL and b"bist_grad_sumsq" in _err()
    assert sumsq(nslots=0) == EINVAL and b"nslots" in _err()
    assert sumsq(nslots=_lib.GRAD_SUMSQ_MAX_SLOTS + 1) == EINVAL and b"nslots" in _err()
    assert sumsq(slot_lo=_lib.GRAD_SUMSQ_MAX_SLOTS - 3) == EINVAL and b"nslots" in _err()
    assert sumsq(a=acc.data_ptr()) == EINVAL and b"together" in _err()
    assert sumsq(ph=phase.data_ptr()) == EINVAL and b"together" in _err()
    hyper = _hyper()
    ctr = torch.zeros(1, device="cuda", dtype=torch.int64)

    def clip(part=slab.data_ptr(), ns=8, max_norm=1.0, h=hyper.data_ptr(), c=ctr.data_ptr()):
        return L.bist_clip_hyper(part, ns, max_norm, h, c, None, st)
    assert clip(part=None) == EINVAL and b"bist_clip_hyper" in _err()
    assert clip(h=None) == EINVAL and b"bist_clip_hyper" in _err()
    assert clip(c=None) == EINVAL and b"bist_clip_hyper" in _err()
    assert clip(ns=0) == EINVAL and b"nslots_total" in _err()
    assert clip(ns=_lib.GRAD_SUMSQ_MAX_SLOTS + 1) == EINVAL and b"nslots_total" in _err()
    for bad in (0.0, -1.0, float("nan")):
        assert clip(max_norm=bad) == EINVAL and b"max_norm" in _err()
    s = _State(1028, torch.bfloat16)
    g = _data(1028, torch.bfloat16, seed=11)
    args = (_ptr(s.m), _ptr(s.v), _ptr(s.work), s.n)
    tail = (B1, B2, EPS, 1, 1, 0, st)
    assert L.bist_adam_step_dev_guard(_ptr(s.p), _ptr(g), *args, None, *tail) == EINVAL and b"bist_adam_step_dev_guard" in _err()
    assert L.bist_adam_accum_dev_guard(_ptr(s.p), _ptr(g), None, *args, s.hyper.data_ptr(), s.phase.data_ptr(), *tail) == EINVAL
    assert b"bist_adam_accum_dev_guard" in _err()
    torch.cuda.synchronize()
    assert torch.isnan(slab).all() and torch.equal(hyper, _hyper()) and int(ctr) == 0
