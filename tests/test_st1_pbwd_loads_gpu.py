"""st1_pbwd_kernel (bist_st_stage1_pv_bwd_p: the stage-1 backward core on SAVED probabilities) after its dO tile and mask bytes became
clamped, unconditional loads issued with the rest of the operand batch: rows >= Lq of the dO tile must still be zeros, keys >= K and
masked keys must still get no score gradient, whatever the query length, key count, group count (workgroups whose last waves exit),
heads, clips, direction, mask and dropout.

Reference: float64, built from the SAME probabilities the kernel is handed and -- with dropout -- the mask recovered from the kernel by
a probe call (P = 1, dO = the identity in each head's first Lq columns: dV then holds mask / (1 - p) element for element).  Bound: 2e-2 of
the largest reference entry, the bound of tests/test_train_gpu.py::test_stage1_backward_bf16_matrix_core_path for dscores and dV."""
import itertools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DK = 64
TOL = 2e-2
DROP = (0.3, 0x51C0FFEE)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from bist_amd import _lib, ops as o
    assert _lib.lib.bist_device_ok() == 1, _lib.lib.bist_last_error()
    return o


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def _close(got, ref, what):
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs().max().item()
    sc = max(1e-3, ref.abs().max().item())
    assert math.isfinite(err) and err <= TOL * sc, f"{what}: err {err:.3e} scale {sc:.3e}"


def _launch(ops, P, V, m8, dO, B, T, S, Lq, h, direction, drop):
    from bist_amd._lib import check, lib
    d, bf = h * DK, torch.bfloat16
    dsc = torch.full((B, Lq * h, T * S), 7.0, device="cuda", dtype=bf)
    dv = torch.full((B, T, S, d), 7.0, device="cuda", dtype=bf)
    check(lib.bist_st_stage1_pv_bwd_p(P.data_ptr(), P.shape[-1], V.data_ptr(), m8.data_ptr() if m8 is not None else None, dO.data_ptr(),
                                      dsc.data_ptr(), ops.dtype_code(bf), dv.data_ptr(), B, T, S, Lq, h, DK, V.stride(-2), d, direction,
                                      ops.drop_ref(drop), ops.dtype_code(bf), torch.cuda.current_stream().cuda_stream), "bist_st_stage1_pv_bwd_p")
    torch.cuda.synchronize()
    return dsc, dv


def _grouped(x, direction):
    """[B, T, S, ...] -> [B, G, K, ...]"""
    return x.transpose(1, 2) if direction == 0 else x


# every value of the issue's table occurs: keys x direction, the other dimensions cycled along
KEYS, LQS, GROUPS, HS, BS, MASKS = [1, 31, 32, 33, 64], [1, 20, 32], [1, 3, 5], [1, 2], [1, 2], ["none", "one", "row"]
CASES = [(K, direction, LQS[n % 3], GROUPS[(n // 2) % 3], HS[n % 2], BS[(n // 3) % 2], MASKS[(n + n // 3) % 3], bool((n // 2) % 2))
         for n, (K, direction) in enumerate(itertools.product(KEYS, (0, 1)))]
CASES += [(33, 0, 32, 5, 2, 2, "one", True), (64, 1, 20, 5, 1, 2, "row", True), (31, 1, 1, 3, 2, 1, "none", False), (1, 0, 20, 5, 2, 2, "row", False)]


@pytest.mark.parametrize("K,direction,Lq,G,h,B,mask,dropout", CASES, ids=lambda v: str(v))
def test_backward_on_saved_probabilities_against_float64(ops, K, direction, Lq, G, h, B, mask, dropout):
    T, S = (K, G) if direction == 0 else (G, K)
    d, bf = h * DK, torch.bfloat16
    KP = (K + 3) // 4 * 4
    live = torch.ones(B, K, dtype=torch.bool)
    if mask == "one":
        live[0, K // 2] = False
    elif mask == "row":
        live[B - 1] = False
    sc = _rand(B, G, h, Lq, K, seed=K + 7 * Lq, scale=2.0).masked_fill(~live.view(B, 1, 1, 1, K), -1e9)
    P = torch.softmax(sc, dim=-1).float()                               # masked keys 0; a fully masked clip uniform (modules.py:60)
    Pp = torch.zeros(B, G, h, Lq, KP)
    Pp[..., :K] = P
    V = _rand(B, T, S, d, seed=61).to(bf)
    dO = _rand(B, G, Lq, d, seed=62).to(bf)
    m8 = live.to(torch.uint8).cuda() if mask != "none" else None
    drop = DROP if dropout else None
    mul = torch.ones(B, G, h, Lq, K, dtype=torch.float64)
    if dropout:
        eye = torch.zeros(B, G, Lq, h, DK)
        for i in range(Lq):
            eye[:, :, i, :, i] = 1.0
        ones = torch.zeros(B, G, h, Lq, KP)
        ones[..., :K] = 1.0
        _, dvp = _launch(ops, ones.cuda(), V.cuda(), None, eye.view(B, G, Lq, d).to(bf).cuda(), B, T, S, Lq, h, direction, drop)
        got = _grouped(dvp.float().cpu(), direction).reshape(B, G, K, h, DK)[..., :Lq]             # [b, g, k, hh, i] = mask / (1 - p)
        keep = got.permute(0, 1, 3, 4, 2) != 0
        if keep.numel() >= 500:
            assert 0.6 < keep.double().mean().item() < 0.8                                          # p = 0.3
        if keep.any():
            assert (got[got != 0] - 1 / (1 - DROP[0])).abs().max().item() < 1e-2
        mul = keep.double() / (1 - DROP[0])
    dsc, dv = _launch(ops, Pp.cuda(), V.cuda(), m8, dO.cuda(), B, T, S, Lq, h, direction, drop)
    # float64 reference
    P6, dO6 = P.double(), dO.double().view(B, G, Lq, h, DK)
    Vg = _grouped(V.double(), direction).reshape(B, G, K, h, DK)
    dP = mul * torch.einsum("bgihc,bgkhc->bghik", dO6, Vg)
    dS = P6 * (dP - (P6 * dP).sum(-1, keepdim=True)) * live.view(B, 1, 1, 1, K)
    dS = dS.permute(0, 3, 2, 4, 1) if direction == 0 else dS.permute(0, 3, 2, 1, 4)               # [B, Lq, h, T, S]
    dVg = torch.einsum("bghik,bgihc->bgkhc", P6 * mul, dO6).reshape(B, G, K, d)
    _close(dsc.view(B, Lq, h, T, S), dS.contiguous(), "dscores")
    _close(dv, _grouped(dVg, direction).contiguous(), "dV")
    if mask != "none":                                                   # masked keys get exactly no score gradient
        dead = _grouped(dsc.view(B, Lq, h, T, S).float().cpu().permute(0, 3, 4, 1, 2), direction)      # [B, G, K, Lq, h]
        assert dead[~live.view(B, 1, K).expand(B, G, K)].abs().max().item() == 0.0
