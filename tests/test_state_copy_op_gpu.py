"""bist_state_copy alone, through the C ABI: the copy, the per-slot digests against the numpy restatement of the
header's definition below, the working-copy cast, and the refusals.

Lengths 1, 2, 7, 8, 9, 1 023, 4 101 and 2^20 + 3: one element (half a word), one word, a scalar tail of three behind one 16-byte group,
exactly one chunk granule, a tail of one, less than a workgroup's first trip with a tail, several trips, many trips with a tail of
three; 1 / 3 / 64 slots (so also more slots than 8-element granules: empty slots); one workgroup per slot and two workgroups walking
all slots.  Every comparison is on bits."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EINVAL = -1                                                       # BIST_EINVAL (include/bist_hip.h)
LENGTHS = [1, 2, 7, 8, 9, 1023, 4101, 2 ** 20 + 3]
NSLOTS = [1, 3, 64]
BLOCKS = [0, 2]
PAD = 8                                                           # sentinel elements behind every destination
SENTINEL = 0x5A5A5A5A
# +-0, +-inf, the smallest and the largest denormal, NaNs with two payloads (one quiet, one signalling with the sign set)
SPECIAL = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x7FC00001, 0xFFA12345], dtype=np.uint32)
M64 = (1 << 64) - 1


def _L():
    from bist_amd import _lib
    return _lib.lib


def _err():
    return _L().bist_last_error()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- the digest of include/bist_hip.h, restated -------------------------------------------------------------------------------------
def word_hashes(bits):
    """h_j of every 64-bit word of a tensor given as uint32 bits (j from 1; an odd length: the last high half is 0)."""
    b = np.concatenate([bits.astype(np.uint64), np.zeros(len(bits) & 1, dtype=np.uint64)])
    with np.errstate(over="ignore"):
        z = (b[0::2] | (b[1::2] << np.uint64(32))) + np.arange(1, len(b) // 2 + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def digest(bits):
    return int(np.add.reduce(word_hashes(bits), dtype=np.uint64))


def slot_digests(bits, nslots):
    """Slot s: the words of elements [s * chunk, min(n, (s + 1) * chunk)), chunk = ceil(n / nslots) rounded up to 8 elements."""
    n, h = len(bits), word_hashes(bits)
    chunk = ((n + nslots - 1) // nslots + 7) // 8 * 8
    out = np.zeros(nslots, dtype=np.uint64)
    for s in range(nslots):
        lo, hi = min(n, s * chunk), min(n, (s + 1) * chunk)
        if lo < hi:                                              # (lo is even: a chunk never splits a word)
            out[s] = np.add.reduce(h[lo // 2:(hi + 1) // 2], dtype=np.uint64)
    return out


def test_the_restatement_wraps_and_sees_flips_and_swaps():
    assert digest(np.array([0, 0], dtype=np.uint32)) == 0xE220A8397B1DCDAF          # splitmix64's first output from state 0
    rs = np.random.RandomState(5)
    x = rs.randint(0, 2 ** 32, size=4101, dtype=np.uint64).astype(np.uint32)
    d = digest(x)
    assert 0 <= d <= M64 and sum(int(v) for v in word_hashes(x)) & M64 == d            # the sum wraps
    y = x.copy(); y[77] ^= 1 << 9
    assert digest(y) != d
    z = x.copy(); z[[10, 11, 20, 21]] = x[[20, 21, 10, 11]]
    assert digest(z) != d


# ---- data -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bits(n, seed):
    """Normal values with the special bit patterns sprinkled in (every one of them where n allows), as uint32."""
    rs = np.random.RandomState(seed)
    x = rs.standard_normal(n).astype(np.float32).view(np.uint32).copy()
    pos = rs.permutation(n)[:min(n, 3 * len(SPECIAL))]
    x[pos] = SPECIAL[np.arange(len(pos)) % len(SPECIAL)]
    x.setflags(write=False)
    return x


def _dev(bits, pad=0):
    """uint32 bits -> a float32 device tensor (pad sentinel elements behind)."""
    full = np.concatenate([bits, np.full(pad, SENTINEL, dtype=np.uint32)])
    return torch.from_numpy(full.view(np.int32).copy()).cuda().view(torch.float32)


def _host(t):
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


def _launch(src, dst, n, nslots, max_blocks=0, work=None, digests=None):
    if digests is None:
        digests = torch.full((3, nslots), -1, device="cuda", dtype=torch.int64)
    d = [None] * 3 if dst is None else [t.data_ptr() for t in dst]
    rc = _L().bist_state_copy(src[0].data_ptr(), src[1].data_ptr(), src[2].data_ptr(), d[0], d[1], d[2],
                              None if work is None else work.data_ptr(), 0 if work is None else int(work.dtype == torch.bfloat16), n,
                              digests.data_ptr(), nslots, max_blocks, _stream())
    assert rc == 0, _err()
    return digests


def _slots(digests):
    return digests.cpu().numpy().view(np.uint64)


# ---- 1. copy and digest against numpy -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_blocks", BLOCKS)
@pytest.mark.parametrize("nslots", NSLOTS)
@pytest.mark.parametrize("n", LENGTHS)
def test_copy_and_slot_digests_against_numpy(n, nslots, max_blocks):
    bits = [_bits(n, seed) for seed in (1, 2, 3)]
    src = [_dev(b) for b in bits]
    dst = [_dev(np.full(n, SENTINEL, dtype=np.uint32), PAD) for _ in range(3)]
    got = _slots(_launch(src, dst, n, nslots, max_blocks))
    chunk = ((n + nslots - 1) // nslots + 7) // 8 * 8
    for i, name in enumerate(("p", "m", "v")):
        out = _host(dst[i])
        assert np.array_equal(out[:n], bits[i]), name
        assert (out[n:] == SENTINEL).all(), "%s: wrote behind its %d elements" % (name, n)
        assert np.array_equal(_host(src[i]), bits[i]), name
        want = slot_digests(bits[i], nslots)
        assert np.array_equal(got[i], want), (name, [s for s in range(nslots) if got[i][s] != want[s]][:4])
        assert int(np.add.reduce(got[i], dtype=np.uint64)) == digest(bits[i]), name
        for s in range(nslots):
            if s * chunk >= n:
                assert got[i][s] == 0, (name, s)
    if n > 8:
        assert len({digest(b) for b in bits}) == 3


# ---- 2. what the digest depends on ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [9, 4101, 2 ** 20 + 3])
def test_the_digest_depends_on_the_bits_and_their_places_only(n):
    bits = [_bits(n, seed) for seed in (1, 2, 3)]
    src = [_dev(b) for b in bits]
    want = [digest(b) for b in bits]

    def totals(d):
        return [int(np.add.reduce(r, dtype=np.uint64)) for r in _slots(d)]
    for nslots in (1, 3, 64, 1000):
        for max_blocks in (0, 2, 7):
            assert totals(_launch(src, None, n, nslots, max_blocks)) == want, (nslots, max_blocks)
    # digest only: the same slots as the copying launch, and nothing else is written
    dst = [_dev(np.full(n, SENTINEL, dtype=np.uint32), PAD) for _ in range(3)]
    copying = _slots(_launch(src, dst, n, 64))
    only = _slots(_launch(src, None, n, 64))
    assert np.array_equal(copying, only)
    for i in range(3):
        assert np.array_equal(_host(src[i]), bits[i])
    # one bit, in the last element (the scalar tail) and in the middle
    for at, bit in ((n - 1, 0), (n // 2, 31)):
        flipped = bits[1].copy(); flipped[at] ^= np.uint32(1 << bit)
        t = totals(_launch([src[0], _dev(flipped), src[2]], None, n, 3))
        assert t[0] == want[0] and t[2] == want[2] and t[1] != want[1] and t[1] == digest(flipped)
    # two unequal word pairs exchanged: the same multiset of words, other places
    a, b = 2, 2 * (n // 4)
    assert not np.array_equal(bits[2][a:a + 2], bits[2][b:b + 2])
    swapped = bits[2].copy(); swapped[a:a + 2], swapped[b:b + 2] = bits[2][b:b + 2], bits[2][a:a + 2]
    t = totals(_launch([src[0], src[1], _dev(swapped)], None, n, 3))
    assert t[:2] == want[:2] and t[2] != want[2] and t[2] == digest(swapped)


# ---- 3. the working copy --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("n", [1, 7, 9, 1023, 4101])
def test_the_working_copy_is_the_cast_of_the_weights(n, dtype):
    rs = np.random.RandomState(9)
    p = (rs.standard_normal(n) * np.exp(rs.uniform(-20, 20, n))).astype(np.float32)          # finite, many exponents
    p[::5] = np.float32(1.0) + np.float32(2.0 ** -8) * rs.randint(0, 4, len(p[::5])).astype(np.float32)      # ties of the bf16 rounding
    bits = [p.view(np.uint32), _bits(n, 2), _bits(n, 3)]
    src = [_dev(b) for b in bits]
    dst = [_dev(np.full(n, SENTINEL, dtype=np.uint32), PAD) for _ in range(3)]
    work = torch.full((n + PAD,), 3.0, device="cuda", dtype=dtype)
    got = _slots(_launch(src, dst, n, 3, work=work))
    want = src[0].to(dtype)
    view = torch.int16 if dtype == torch.bfloat16 else torch.int32
    assert torch.equal(work[:n].view(view), want.view(view))
    assert (work[n:] == 3.0).all()
    for i in range(3):
        assert np.array_equal(_host(dst[i])[:n], bits[i]) and (_host(dst[i])[n:] == SENTINEL).all()
        assert int(np.add.reduce(got[i], dtype=np.uint64)) == digest(bits[i])


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------
def test_bad_calls_are_refused_before_any_launch():
    from bist_amd import _lib
    L = _L()
    n = 64
    src = [_dev(_bits(n + 4, seed)) for seed in (1, 2, 3)]
    dst = [_dev(np.full(n + 4, SENTINEL, dtype=np.uint32)) for _ in range(3)]
    work = torch.full((n + 8,), 3.0, device="cuda", dtype=torch.bfloat16)
    workf = torch.full((n + 8,), 3.0, device="cuda", dtype=torch.float32)
    dig = torch.full((3, 4), -1, device="cuda", dtype=torch.int64)
    st = _stream()
    S, D = [t.data_ptr() for t in src], [t.data_ptr() for t in dst]

    def call(s=S, d=D, w=None, wd=0, n=n, g=dig.data_ptr(), nslots=4, max_blocks=0):
        return L.bist_state_copy(s[0], s[1], s[2], d[0], d[1], d[2], w, wd, n, g, nslots, max_blocks, st)

    def refused(word, **kw):
        assert call(**kw) == EINVAL, kw
        assert b"bist_state_copy" in _err() and word in _err(), (kw, _err())
    for i in range(3):
        refused(b"null", s=S[:i] + [None] + S[i + 1:])
    refused(b"null", g=None)
    refused(b"n must", n=0)
    refused(b"n must", n=-8)
    refused(b"nslots", nslots=0)
    refused(b"nslots", nslots=_lib.STATE_MAX_SLOTS + 1)
    refused(b"max_blocks", max_blocks=-1)
    for keep in ([0], [1], [2], [0, 1], [0, 2], [1, 2]):
        refused(b"together", d=[D[i] if i in keep else None for i in range(3)])
    for i in range(3):
        for j in range(3):
            refused(b"also a dst", d=D[:j] + [S[i]] + D[j + 1:])
    for i in range(3):
        refused(b"aligned", s=S[:i] + [S[i] + 4] + S[i + 1:])
        refused(b"aligned", d=D[:i] + [D[i] + 8] + D[i + 1:])
    refused(b"aligned", g=dig.data_ptr() + 4)
    refused(b"aligned", w=work.data_ptr() + 4, wd=1)
    refused(b"aligned", w=workf.data_ptr() + 8, wd=0)
    refused(b"work_dtype", w=work.data_ptr(), wd=2)
    refused(b"work_dtype", w=work.data_ptr(), wd=-1)
    torch.cuda.synchronize()
    for t in dst:
        assert (_host(t) == SENTINEL).all()
    assert (work == 3.0).all() and (workf == 3.0).all() and (dig == -1).all()
    assert call() == 0 and call(w=work.data_ptr() + 8, wd=1) == 0 and call(d=[None] * 3) == 0          # (the accepted forms of the same call)
    torch.cuda.synchronize()
    assert np.array_equal(_host(dst[0])[:n], _bits(n + 4, 1)[:n]) and (_host(dst[0])[n:] == SENTINEL).all()
