"""Outputs of the three attention cores (stage 2 on the matrix cores, small attention forward, small attention backward on
the matrix cores), forward and backward, for seeded inputs at the shapes of tests/test_attention_loads_gpu.py, and of the stage-1
backward core on saved probabilities (st1_pbwd_kernel) at the shapes of tests/test_st1_pbwd_loads_gpu.py plus bench.py's:

    python scripts/dump_attention_cores.py DIR            one .npy of raw bytes per case under DIR
    python scripts/dump_attention_cores.py --compare A B  numpy.array_equal on every file of two such directories

A change that only moves when operands are fetched must leave every file identical; run it in both trees and compare."""
import json
import os
import sys

import numpy as np

ST2_G = [1, 2, 31, 32, 33, 48, 49, 55, 56, 57, 63, 64, 65, 127, 128]
ST2_SHAPES = [(1, 1, 1, 128), (2, 3, 5, 256), (3, 20, 8, 512), (16, 20, 8, 512)]
MHA_SHAPES = [(1, 1, 1, 1, 64), (3, 20, 20, 8, 64), (2, 20, 25, 8, 64), (2, 20, 60, 8, 64), (2, 20, 64, 8, 64), (2, 6, 130, 1, 64),
              (4, 20, 25, 1, 512), (2, 5, 7, 4, 16), (2, 4, 11, 2, 32), (16, 20, 20, 8, 64)]


# (keys, direction, Lq, groups, h, B, mask, dropout): tests/test_st1_pbwd_loads_gpu.py::CASES, then the bench shapes (B = 16, T = 32, S = 49)
PBWD_KEYS, PBWD_LQ, PBWD_G, PBWD_MASKS = [1, 31, 32, 33, 64], [1, 20, 32], [1, 3, 5], ["none", "one", "row"]
PBWD_CASES = [(K, dr, PBWD_LQ[n % 3], PBWD_G[(n // 2) % 3], [1, 2][n % 2], [1, 2][(n // 3) % 2], PBWD_MASKS[(n + n // 3) % 3], bool((n // 2) % 2))
              for n, (K, dr) in enumerate((K, dr) for K in PBWD_KEYS for dr in (0, 1))]
PBWD_CASES += [(33, 0, 32, 5, 2, 2, "one", True), (64, 1, 20, 5, 1, 2, "row", True), (31, 1, 1, 3, 2, 1, "none", False), (1, 0, 20, 5, 2, 2, "row", False)]
PBWD_CASES += [(32, 0, 20, 49, 8, 16, "one", True), (49, 1, 20, 32, 8, 16, "none", True), (32, 0, 20, 49, 8, 16, "row", False), (49, 1, 20, 32, 8, 16, "none", False)]


def compare(a, b):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    bad = [f for f in fa if f not in fb] + [f for f in fb if f not in fa]
    for f in fa:
        if f in fb and not np.array_equal(np.load(os.path.join(a, f)), np.load(os.path.join(b, f))):
            bad.append(f)
    print(json.dumps({"files": len(fa), "equal": not bad, "different": bad}))
    return 0 if not bad else 1


def main(out):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bist_amd import functional as Fn, ops
    os.makedirs(out, exist_ok=True)
    bf = torch.bfloat16

    def rand(*shape, seed, scale=1.0):
        return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale

    def save(name, tensors):
        raw = [t.detach().contiguous().view(torch.uint8).flatten().cpu().numpy() for t in tensors if t is not None]
        np.save(os.path.join(out, name + ".npy"), np.concatenate(raw))

    def st2_mask(kind, B, G):
        if kind == "none":
            return None
        gm = torch.ones(B, 1, G, dtype=torch.bool)
        if kind == "tail":
            gm[0, 0, G // 3:] = False
        else:
            gm[B - 1] = False
        return gm.cuda()

    def attn_mask(kind, N, Lq, Lk):
        if kind == "key":
            m = torch.ones(N, 1, Lk, dtype=torch.bool)
            m[0, 0, Lk // 2:] = False
            m[N - 1] = False
            return m.cuda()
        if kind == "causal":
            return torch.tril(torch.ones(1, Lq, Lk, dtype=torch.bool)).expand(N, Lq, Lk).clone().cuda()
        return None

    for (B, Lq, h, d) in ST2_SHAPES:
        for G in ST2_G:
            q2f = rand(B, Lq, h, d, seed=70, scale=d ** -0.5).to(bf).cuda()
            y = rand(B, G, Lq, d, seed=71).to(bf).cuda()
            go = rand(B, Lq, h, d, seed=72).to(bf).cuda()
            for kind, drop in (("none", None), ("tail", None), ("clip", None), ("tail", (0.1, 1234))):
                qd, yd = q2f.clone().requires_grad_(True), y.clone().requires_grad_(True)
                o, rs = Fn.st_stage2(qd, yd, st2_mask(kind, B, G), h=h, drop=drop)
                o.backward(go)
                save(f"st2_B{B}_Lq{Lq}_h{h}_d{d}_G{G}_{kind}_{'drop' if drop else 'nodrop'}", [o, rs, qd.grad, yd.grad])

    for (N, Lq, Lk, h, dk) in MHA_SHAPES:
        d, L = h * dk, max(Lq, Lk)
        for dtype in (bf, torch.float32):
            buf = rand(N, L, 3 * d, seed=16).to(dtype).cuda()
            q, k, v = buf[:, :Lq, :d], buf[:, :Lk, d:2 * d], buf[:, :Lk, 2 * d:]
            for kind, want_p, drop in (("key", False, None), ("causal", False, None), ("none", False, None), ("key", True, None),
                                       ("key", True, (0.1, 77))):
                o, p = ops.mha_core(q, k, v, attn_mask(kind, N, Lq, Lk), h, want_p=want_p, drop=drop)
                save(f"mha_fwd_N{N}_Lq{Lq}_Lk{Lk}_h{h}_dk{dk}_{'bf16' if dtype == bf else 'f32'}_{kind}_p{int(want_p)}_{'drop' if drop else 'nodrop'}",
                     [o, p])

    for Lk in (1, 7, 8, 9, 20, 25, 60, 63, 64):
        for Lq in (1, 20, 32):
            for h in (1, 8):
                for dk in (64, 192):
                    N, d = 2, h * dk
                    q = rand(N, Lq, d, seed=80, scale=(64.0 / dk) ** 0.5).to(bf).cuda()
                    kv = rand(N, Lk, 2 * d, seed=81).to(bf).cuda()
                    wo, wp = rand(N, Lq, d, seed=82).to(bf).cuda(), rand(N, h, Lq, Lk, seed=83).float().cuda()
                    for kind in ("key", "causal", "none"):
                        qd, kvd = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
                        o, p = Fn.mha_packed(qd, kvd, None, "q_kv", attn_mask(kind, N, Lq, Lk), h, True)
                        ((o.float() * wo.float()).sum() + (p * wp).sum()).backward()
                        save(f"mha_bwd_Lk{Lk}_Lq{Lq}_h{h}_dk{dk}_{kind}", [o, p, qd.grad, kvd.grad])
    from bist_amd._lib import check, lib
    for (K, direction, Lq, G, h, B, mask, dropout) in PBWD_CASES:
        T, S = (K, G) if direction == 0 else (G, K)
        d, KP = h * 64, (K + 3) // 4 * 4
        live = torch.ones(B, K, dtype=torch.bool)
        if mask == "one":
            live[0, K // 2] = False
        elif mask == "row":
            live[B - 1] = False
        sc = rand(B, G, h, Lq, K, seed=90, scale=2.0).masked_fill(~live.view(B, 1, 1, 1, K), -1e9)
        P = torch.zeros(B, G, h, Lq, KP)
        P[..., :K] = torch.softmax(sc, dim=-1).float()
        P, V, dO = P.cuda(), rand(B, T, S, d, seed=91).to(bf).cuda(), rand(B, G, Lq, d, seed=92).to(bf).cuda()
        m8 = live.to(torch.uint8).cuda() if mask != "none" else None
        dsc = torch.zeros(B, Lq * h, T * S, device="cuda", dtype=bf)
        dv = torch.zeros(B, T, S, d, device="cuda", dtype=bf)
        check(lib.bist_st_stage1_pv_bwd_p(P.data_ptr(), KP, V.data_ptr(), m8.data_ptr() if m8 is not None else None, dO.data_ptr(), dsc.data_ptr(),
                                          ops.dtype_code(bf), dv.data_ptr(), B, T, S, Lq, h, 64, V.stride(-2), d, direction,
                                          ops.drop_ref((0.3, 4321) if dropout else None), ops.dtype_code(bf), torch.cuda.current_stream().cuda_stream),
              "bist_st_stage1_pv_bwd_p")
        save(f"st1_pbwd_K{K}_dir{direction}_Lq{Lq}_G{G}_h{h}_B{B}_{mask}_{'drop' if dropout else 'nodrop'}", [dsc, dv])
    torch.cuda.synchronize()
    print(json.dumps({"dir": out, "files": len(os.listdir(out))}))
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1]))
