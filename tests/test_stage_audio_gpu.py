"""bist_stage_audio (csrc/stage_audio.hip): audio features [B, Ta, Da] staged into a class buffer [B, PTa >= Ta, Da] in the compute dtype
with audio_mask [B, 1, PTa] -- bit-identical to padding the SOURCE with zero rows on the host and then building the Batch
(data/dataset.py:83-87: audio_mask = (audio_fts.sum(-1) != 0).unsqueeze(-2); on the device Batch derives it with bist_temporal_mask,
row_elems = Da, whose per-row summation order the staging launch reproduces) and casting the features.

Every source holds an all-zero row and a row whose entries are non-zero yet sum to exactly 0.0 (+1, -1, 0, ...): both must come out
masked, exactly where Batch masks them.  Da = 10 rows are neither whole 16-byte vectors of f32 nor of bf16: the launch's scalar path.
The destination and the mask lie inside larger poisoned buffers: nothing beyond [B, PTa, Da] / [B, PTa] may be written."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 3


def _next_rung(Ta):
    from bist_amd.data.classes import LengthClasses
    return LengthClasses().round("audio", Ta if Ta % 16 else Ta + 1)       # 16 -- or, from a length that is a rung already, the next one


def _source(Ta, Da, dtype):
    g = torch.Generator().manual_seed(100 * Ta + Da)
    au = torch.randn(B, Ta, Da, generator=g)
    if Ta > 1:
        au[1, Ta - 1] = 0.0                                 # an all-zero row
        au[2, Ta // 2:] = 0.0                               # a zero tail
    zr = min(2, Ta - 1)
    au[0, zr] = 0.0
    au[0, zr, 0], au[0, zr, 1] = 1.0, -1.0                  # non-zero entries that sum to exactly 0.0 (exact in bf16 too)
    return au.to(dtype), zr


@pytest.mark.parametrize("src_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("Da", [128, 16, 10])
@pytest.mark.parametrize("pta", ["same", "rung", 64])
@pytest.mark.parametrize("Ta", [1, 9, 33])
def test_staged_audio_equals_host_padding_then_batch(Ta, pta, Da, src_dtype):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from bist_amd import ops
    from bist_amd.data.batch import Batch
    PTa = Ta if pta == "same" else _next_rung(Ta) if pta == "rung" else 64
    assert PTa >= Ta
    src, zr = _source(Ta, Da, src_dtype)
    padded = torch.cat([src, torch.zeros(B, PTa - Ta, Da, dtype=src_dtype)], 1)              # host padding ...
    ids = torch.full((B, 2), 5, dtype=torch.int64)
    host = Batch(ids, ids, None, None, ids, ids, audio_fts=padded)                           # ... then Batch: on the host,
    dev = Batch(ids.cuda(), ids.cuda(), None, None, ids.cuda(), ids.cuda(), audio_fts=[padded.cuda()])      # and on the device
    assert torch.equal(dev.audio_mask.cpu(), host.audio_mask)
    want_mask = host.audio_mask
    assert not want_mask[0, 0, zr] and not want_mask[:, 0, Ta:].any()
    assert want_mask[0, 0, 0] or zr == 0
    s = src.cuda()
    for out_dtype in (torch.bfloat16, torch.float32):
        poison = 96.0
        flat = torch.full((B * PTa * Da + 64,), poison, dtype=out_dtype, device="cuda")
        mflat = torch.full((B * PTa + 64,), 7, dtype=torch.uint8, device="cuda")
        dst = flat[:B * PTa * Da].view(B, PTa, Da)
        mask = mflat[:B * PTa].view(torch.bool).view(B, 1, PTa)
        ops.stage_audio(s, dst, mask)
        torch.cuda.synchronize()
        want = padded.to(out_dtype)
        bits = torch.int16 if out_dtype == torch.bfloat16 else torch.int32                   # (bits: -0.0 and 0.0 are told apart)
        assert torch.equal(dst.cpu().contiguous().view(bits), want.contiguous().view(bits)), (out_dtype, "feature bits")
        assert torch.equal(mflat[:B * PTa].cpu(), want_mask.reshape(-1).to(torch.uint8)), (out_dtype, "mask bytes")
        assert (flat[B * PTa * Da:] == poison).all() and (mflat[B * PTa:] == 7).all(), (out_dtype, "written past the end")
        # the staged buffer seen as a Batch of its own: the same mask (a zero tail row is masked by construction)
        if out_dtype == src_dtype:
            assert torch.equal(ops.audio_mask(dst).cpu(), want_mask)


def test_bad_arguments_are_refused():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from bist_amd import ops
    src = torch.zeros(B, 9, 16, device="cuda")
    with pytest.raises(ValueError):
        ops.stage_audio(src, torch.zeros(B, 8, 16, device="cuda"), torch.zeros(B, 1, 8, dtype=torch.bool, device="cuda"))      # PTa < Ta
    with pytest.raises(ValueError):
        ops.stage_audio(src, torch.zeros(B, 16, 8, device="cuda"), torch.zeros(B, 1, 16, dtype=torch.bool, device="cuda"))     # another width
    with pytest.raises(ValueError):
        ops.stage_audio(src, torch.zeros(B, 16, 16, device="cuda"), torch.zeros(B, 16, dtype=torch.bool, device="cuda"))       # mask shape
