"""bist_stage_train_batch against a torch restatement of the reference's padding: ``F.pad`` of every token tensor with the pad id and of
the features with zero frames, then ``bist_amd.data.Batch`` on the padded tensors -- bit for bit, every field, inside guard bands that the
launch must leave untouched."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

PAD = 1
GUARD = 4096
SENT = {torch.int64: 0x5A5A5A5A5A5A5A5A, torch.uint8: 0xAB}


def _ragged(B, L, rs, vocab=80, pad_rows=True):
    x = rs.randint(4, vocab, size=(B, L)).astype(np.int64)
    if pad_rows:
        for i in range(B):
            if rs.rand() < 0.4 and L > 1:
                x[i, int(rs.randint(1, L)):] = PAD
    return torch.from_numpy(x).cuda()


def _src(B, Lq, Lh, Lc, Lt, T, S, C, dtype, seed, cap=True, strided=False):
    from bist_amd.data.batch import Batch
    rs = np.random.RandomState(seed)
    fts = torch.from_numpy(rs.standard_normal((B, T, S, C)).astype(np.float32))
    for i in range(B):
        fts[i, int(rs.randint(max(1, T // 2), T + 1)):] = 0.0          # zero frames INSIDE the exact length
    if T > 2:
        fts[0, 1] = 0.0
        fts[0, 1, 0, 0], fts[0, 1, 0, 1] = 1.0, -1.0                      # a frame whose features cancel: sum 0, mask False
    q, h = _ragged(B, Lq, rs), _ragged(B, Lh, rs)
    c = _ragged(B, Lc, rs) if cap else None
    full = _ragged(B, Lt + 1, rs)
    if strided:                                                           # token rows that are views of a wider tensor
        trg, trg_y = full[:, :-1], full[:, 1:]
    else:
        trg, trg_y = full[:, :-1].clone(), full[:, 1:].clone()
    return Batch(q, h, fts.to(dtype).cuda(), c, trg, trg_y, pad=PAD)


def _guarded(shape, dtype, keep):
    n = 1
    for s in shape:
        n *= s
    if dtype == torch.bool:
        buf = torch.full((n + 2 * GUARD,), SENT[torch.uint8], dtype=torch.uint8, device="cuda")
        t = buf[GUARD:GUARD + n].view(torch.bool).view(shape)
    elif dtype == torch.int64:
        buf = torch.full((n + 2 * GUARD,), SENT[torch.int64], dtype=torch.int64, device="cuda")
        t = buf[GUARD:GUARD + n].view(shape)
    else:
        buf = torch.full((n + 2 * GUARD,), 7.0, dtype=dtype, device="cuda")
        t = buf[GUARD:GUARD + n].view(shape)
    keep.append((buf, buf.clone()))
    return t


def _dst(src, P, out_dtype, keep):
    import copy
    B = src.query.shape[0]
    d = copy.copy(src)
    d.query, d.his, d.trg = (_guarded((B, P[k]), torch.int64, keep) for k in ("query", "his", "trg"))
    d.trg_y = _guarded((B, P["trg"]), torch.int64, keep)
    d.cap = _guarded((B, P["cap"]), torch.int64, keep) if src.cap is not None else None
    d.fts = _guarded((B, P["frames"]) + tuple(src.fts.shape[2:]), out_dtype, keep)
    d.query_mask, d.query_mask2 = _guarded((B, 1, P["query"]), torch.bool, keep), _guarded((2 * B, 1, P["query"]), torch.bool, keep)
    d.his_mask = _guarded((B, 1, P["his"]), torch.bool, keep)
    d.cap_mask = _guarded((B, 1, P["cap"]), torch.bool, keep) if src.cap is not None else None
    d.trg_mask, d.trg_mean_mask = _guarded((B, P["trg"], P["trg"]), torch.bool, keep), _guarded((B, P["trg"]), torch.bool, keep)
    d.temporal_mask = _guarded((B, 1, P["frames"]), torch.bool, keep)
    d.ntokens, d.qntokens = _guarded((), torch.int64, keep), _guarded((), torch.int64, keep)
    return d


def _restated(src, P, out_dtype):
    from bist_amd.data.batch import Batch

    def pad_ids(t, L):
        return F.pad(t, (0, L - t.shape[1]), value=PAD) if t is not None else None
    f = src.fts.to(out_dtype)
    f = F.pad(f, (0, 0, 0, 0, 0, P["frames"] - f.shape[1]))
    return Batch(pad_ids(src.query, P["query"]), pad_ids(src.his, P["his"]), f, pad_ids(src.cap, P["cap"]),
                 pad_ids(src.trg, P["trg"]), pad_ids(src.trg_y, P["trg"]), pad=PAD)


FIELDS = ("query", "his", "cap", "trg", "trg_y", "fts", "query_mask", "query_mask2", "his_mask", "cap_mask", "trg_mask", "trg_mean_mask",
          "temporal_mask", "ntokens", "qntokens")

CASES = [
    # B, Lq, Lh, Lc, Lt, T, S, C, in dtype, out dtype, cap, strided ids
    (4, 7, 9, 6, 6, 6, 9, 64, torch.float32, torch.float32, True, False),
    (3, 20, 60, 25, 20, 32, 9, 64, torch.float32, torch.bfloat16, True, True),
    (5, 13, 33, 17, 9, 19, 49, 128, torch.bfloat16, torch.bfloat16, True, False),
    (2, 1, 1, 1, 1, 1, 9, 64, torch.bfloat16, torch.float32, True, False),
    (7, 30, 100, 40, 31, 40, 49, 64, torch.float32, torch.bfloat16, False, False),
    (32, 24, 64, 32, 24, 32, 49, 256, torch.float32, torch.bfloat16, True, False),
    (32, 9, 77, 50, 17, 63, 9, 64, torch.bfloat16, torch.bfloat16, True, True),
]


@pytest.mark.parametrize("case", CASES, ids=[f"B{c[0]}-T{c[5]}-{str(c[8])[6:]}-{str(c[9])[6:]}" for c in CASES])
@pytest.mark.parametrize("extra", [0, 1])
def test_stage_train_batch_equals_pad_then_batch(case, extra):
    from bist_amd import ops
    from bist_amd.data.classes import LengthClasses
    B, Lq, Lh, Lc, Lt, T, S, C, din, dout, cap, strided = case
    src = _src(B, Lq, Lh, Lc, Lt, T, S, C, din, seed=1000 + 17 * B + T + extra, cap=cap, strided=strided)
    P = LengthClasses().shape(src)
    if extra:                                  # a class longer than the ladder's: more padding everywhere
        P = {k: (v + 5 if v is not None else None) for k, v in P.items()}
    if cap is False:
        P["cap"] = 8
    keep = []
    dst = _dst(src, P, dout, keep)
    ops.stage_train_batch(src, dst, PAD)
    ref = _restated(src, P, dout)
    torch.cuda.synchronize()
    for f in FIELDS:
        a, b = getattr(dst, f), getattr(ref, f)
        if b is None:
            assert f in ("cap", "cap_mask") and not cap
            continue
        assert a.shape == b.shape and a.dtype == b.dtype, (f, a.shape, b.shape, a.dtype, b.dtype)
        if a.is_floating_point():
            assert torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32),
                               b.contiguous().view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32)), f
        else:
            assert torch.equal(a, b), f
    assert not bool(dst.temporal_mask[0, 0, 1]) or T <= 2
    for buf, orig in keep:                       # nothing written outside the class buffers
        assert torch.equal(buf[:GUARD], orig[:GUARD]) and torch.equal(buf[-GUARD:], orig[-GUARD:])


def test_stage_train_batch_refuses_a_class_shorter_than_the_batch():
    from bist_amd import ops
    src = _src(2, 7, 9, 6, 6, 6, 9, 64, torch.float32, seed=5)
    keep = []
    dst = _dst(src, {"query": 4, "his": 16, "cap": 8, "trg": 8, "frames": 8}, torch.float32, keep)
    with pytest.raises(ValueError):
        ops.stage_train_batch(src, dst, PAD)
    dst = _dst(src, {"query": 8, "his": 16, "cap": 8, "trg": 8, "frames": 4}, torch.float32, keep)
    with pytest.raises(ValueError):
        ops.stage_train_batch(src, dst, PAD)


@pytest.mark.parametrize("name,shape", [("query_mask2", lambda B, P: (B, 1, P["query"])), ("trg_mask", lambda B, P: (B, P["trg"], P["trg"] - 1)),
                                        ("trg_mean_mask", lambda B, P: (B, P["trg"] + 1)), ("temporal_mask", lambda B, P: (B, 1, P["frames"] - 1)),
                                        ("his_mask", lambda B, P: (B, P["his"]))])
def test_stage_train_batch_refuses_a_mask_of_the_wrong_shape(name, shape):
    """The launch writes the masks through raw pointers: a destination mask of any other shape than Batch's at the class lengths is refused."""
    from bist_amd import ops
    src = _src(3, 7, 9, 6, 6, 6, 9, 64, torch.float32, seed=7)
    P = {"query": 8, "his": 16, "cap": 8, "trg": 8, "frames": 8}
    keep = []
    dst = _dst(src, P, torch.float32, keep)
    setattr(dst, name, _guarded(shape(3, P), torch.bool, keep))
    with pytest.raises(ValueError):
        ops.stage_train_batch(src, dst, PAD)
    dst = _dst(src, P, torch.float32, keep)
    dst.trg_mask = None
    with pytest.raises(ValueError):
        ops.stage_train_batch(src, dst, PAD)
