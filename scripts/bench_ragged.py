"""Training on ragged batches: today's exact-shape graphs against length classes, at BASELINE configs[1] model size.

Seeded synthetic batches with AVSD-like per-clip lengths -- query, history, caption, answer and frames drawn per clip, then every batch
padded to its own maxima as the reference's collate_fn does (data/dataset.py:133-195) -- so nearly every batch has a new exact geometry.

  python scripts/bench_ragged.py [--steps 200] [--rounds 2] [--out profiles/ragged_classes.json]
      modes alternated in one process, `rounds` blocks each of steps / rounds batches:
        exact    Trainer(use_graph=True): one graph keyed by the exact shape -- ms per step, captures
        classes  Trainer(use_graph=True, length_classes=LengthClasses()): ms per step over all steps, steady state (median of the steps
                 that replayed a stored class), distinct class keys, captures, bytes per entry and in total
      then the cost of padding at the bench geometry (B=16, T=32, Lq=20, Lh=60, Lc=25, Lt=20): the exact replayed step (resident batch,
      as bench.py times it) against the class-mode step at its class (24/64/32/24/32: staged and padded every step) and against a
      one-class ladder of exactly the bench geometry (staged every step, nothing padded), and the staging launch against a device copy
      of the same bytes (HIP events).
  python scripts/bench_ragged.py --stage-only [--iters 50]
      only the staging launch and the device copy, for `rocprofv3 --kernel-trace --stats -- python scripts/bench_ragged.py --stage-only`.

Every step is followed by a device synchronisation in the ragged sequence (so that a step's time is its own: captures and replays
alike); the bench-geometry loops are not (as bench.py).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (sets the HIP runtime switches of the split executor before the runtime starts)


def clip_lengths(rs, B):
    """AVSD-like per-clip lengths (questions ~10 tokens, three turns of history, caption + summary, answers ~12 tokens, 16..32 segments)."""
    q = np.minimum(3 + rs.poisson(7, B), 30)
    h = np.minimum(10 + rs.poisson(45, B), 150)
    c = np.minimum(8 + rs.poisson(22, B), 60)
    t = np.minimum(3 + rs.poisson(9, B), 30)
    T = rs.randint(16, 33, B)
    return q, h, c, t, T


def ragged_batches(n, seed, c, dtype, pool):
    """n device batches; each padded to its own maxima (collate_fn), ids uniform, features from a device pool with zero frames past each clip."""
    from bist_amd.data.batch import PAD, Batch
    from bist_amd.data.synthetic import EOS, SOS
    rs = np.random.RandomState(seed)
    out = []
    B = c["B"]
    for i in range(n):
        q, h, cp, t, T = clip_lengths(rs, B)

        def ids(lens):
            x = np.full((B, int(lens.max())), PAD, dtype=np.int64)
            for r, L in enumerate(lens):
                x[r, :L] = rs.randint(4, c["V"], L)
            return torch.from_numpy(x).cuda()
        full = np.full((B, int(t.max()) + 1), PAD, dtype=np.int64)
        for r, L in enumerate(t):
            full[r, 0] = SOS
            full[r, 1:L] = rs.randint(4, c["V"], L - 1)
            full[r, L] = EOS
        full = torch.from_numpy(full).cuda()
        fts = pool[i % len(pool)][:, :int(T.max())].clone()
        for r, L in enumerate(T):
            fts[r, int(L):] = 0
        out.append(Batch(ids(q), ids(h), fts, ids(cp), full[:, :-1].contiguous(), full[:, 1:].contiguous(), pad=PAD))
    return out


def stage_rate(c, iters):
    """The staging launch on the bench geometry (fp32 features in, bf16 out, class = exact) against a device copy of the same bytes."""
    import copy as _copy
    from bist_amd import ops
    from bist_amd.data.classes import LengthClasses
    from bist_amd.data.synthetic import synthetic_batch
    src = synthetic_batch(c["B"], T=c["T"], S=c["S"], C=c["C"], Lq=c["Lq"], Lh=c["Lh"], Lc=c["Lc"], Lt=c["Lt"], vocab=c["V"], seed=1234,
                          dtype=torch.float32)
    shp = LengthClasses().shape(src)
    B = c["B"]
    dst = _copy.copy(src)
    dev = "cuda"
    dst.query, dst.his, dst.cap = (torch.empty(B, shp[k], dtype=torch.int64, device=dev) for k in ("query", "his", "cap"))
    dst.trg, dst.trg_y = (torch.empty(B, shp["trg"], dtype=torch.int64, device=dev) for _ in range(2))
    dst.fts = torch.empty(B, shp["frames"], c["S"], c["C"], dtype=torch.bfloat16, device=dev)
    mk = lambda *s: torch.empty(*s, dtype=torch.bool, device=dev)  # noqa: E731
    dst.query_mask, dst.query_mask2, dst.his_mask, dst.cap_mask = mk(B, 1, shp["query"]), mk(2 * B, 1, shp["query"]), mk(B, 1, shp["his"]), mk(B, 1, shp["cap"])
    dst.trg_mask, dst.trg_mean_mask, dst.temporal_mask = mk(B, shp["trg"], shp["trg"]), mk(B, shp["trg"]), mk(B, 1, shp["frames"])
    dst.ntokens, dst.qntokens = torch.zeros((), dtype=torch.int64, device=dev), torch.zeros((), dtype=torch.int64, device=dev)
    moved = src.fts.numel() * 4 + dst.fts.numel() * 2             # features read + written (ids and masks: a few kB)
    a = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)

    def timed(fn):
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters
    res = {}
    for rep in range(2):                                            # alternated
        st = timed(lambda: ops.stage_train_batch(src, dst, 1))
        cp = timed(lambda: b.copy_(a))
        res.setdefault("stage_ms", []).append(st)
        res.setdefault("copy_ms", []).append(cp)
    st, cp = min(res["stage_ms"]), min(res["copy_ms"])
    res.update(bytes_moved=moved, stage_TBps=moved / st / 1e9, copy_TBps=moved / cp / 1e9, stage_over_copy=cp / st,
               geometry={"B": B, "T": c["T"], "S": c["S"], "C": c["C"], "in": "float32", "out": "bfloat16"})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--bench-steps", type=int, default=30)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--stage-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    c = dict(bench.CFG)
    if a.stage_only:
        print(json.dumps({"stage": stage_rate(c, a.iters)}))
        return

    import bist_amd.model as M
    from bist_amd import functional as Fn, ops
    from bist_amd.data.classes import LengthClasses
    from bist_amd.data.synthetic import synthetic_batch
    from bist_amd.train import Trainer
    if Fn.main_stream() is not None:
        torch.cuda.set_stream(Fn.main_stream())
    dtype = torch.bfloat16
    args = bench.model_args(c["L"], c["d"], c["h"], 0.1)
    g = torch.Generator(device="cuda").manual_seed(7)
    pool = [torch.randn(c["B"], c["T"], c["S"], c["C"], generator=g, device="cuda", dtype=torch.float32).to(dtype) for _ in range(4)]
    batches = ragged_batches(a.steps, 2024, c, dtype, pool)
    del pool

    def trainer(**kw):
        torch.manual_seed(1)
        model = M.make_model(c["V"], c["V"], args, ft_sizes=[c["C"]]).cuda()
        model.train()
        Fn.manual_seed(1234)
        return Trainer(model, args, c["V"], compute_dtype=dtype, use_graph=True, **kw)
    lc = LengthClasses()
    tr_e, tr_c = trainer(), trainer(length_classes=lc)
    n_cap = [0]
    orig_capture = tr_e._capture

    def counted(*x):
        n_cap[0] += 1
        return orig_capture(*x)
    tr_e._capture = counted
    t_e, t_c, hit_c = [], [], []
    per = a.steps // a.rounds
    for r in range(a.rounds):
        part = batches[r * per:(r + 1) * per]
        for tr, times in ((tr_e, t_e), (tr_c, t_c)):
            ops.DROP_CTR = tr.drop_ctr
            for bt in part:
                before = tr.graph_stats()["captures"]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tr.step(bt)
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
                if tr is tr_c:
                    hit_c.append(tr.graph_stats()["captures"] == before)
            print("round %d %s: %d steps, %.1f ms per step" % (r, "classes" if tr is tr_c else "exact", len(part),
                                                              1e3 * sum(times[-len(part):]) / len(part)), file=sys.stderr, flush=True)
    keys = {lc.key(bt) for bt in batches}
    exact_keys = {tuple((f, tuple(getattr(bt, f).shape)) for f in ("query", "his", "cap", "trg", "fts")) for bt in batches}
    st = tr_c.graph_stats()
    per_entry = [e.bytes for e in tr_c._entries.values()]
    hits = [t for t, h in zip(t_c, hit_c) if h]
    caps = [t for t, h in zip(t_c, hit_c) if not h]
    out = {
        "config": {"B": c["B"], "S": c["S"], "C": c["C"], "L": c["L"], "d": c["d"], "steps": a.steps, "rounds": a.rounds, "dtype": "bf16",
                   "ladder": repr(lc), "max_graphs": tr_c.max_graphs},
        "exact": {"ms_per_step": 1e3 * sum(t_e) / len(t_e), "captures": n_cap[0], "distinct_exact_geometries": len(exact_keys),
                  "median_ms": 1e3 * float(np.median(t_e))},
        "classes": {"ms_per_step": 1e3 * sum(t_c) / len(t_c), "steady_ms_per_step": 1e3 * float(np.median(hits)) if hits else None,
                    "steady_mean_ms": 1e3 * float(np.mean(hits)) if hits else None,
                    "capture_step_ms_median": 1e3 * float(np.median(caps)) if caps else None,
                    "distinct_class_keys": len(keys), "captures": st["captures"], "hits": st["hits"], "evictions": st["evictions"],
                    "entries": st["entries"], "bytes_total": st["bytes"], "bytes_per_entry": per_entry},
    }
    print(json.dumps(out), flush=True)

    # ---- the cost of padding at the bench geometry -------------------------------------------------------------------------------
    bb = synthetic_batch(c["B"], T=c["T"], S=c["S"], C=c["C"], Lq=c["Lq"], Lh=c["Lh"], Lc=c["Lc"], Lt=c["Lt"], vocab=c["V"], seed=1234,
                         dtype=dtype)
    del batches
    tr_f = trainer(length_classes=LengthClasses.fixed(query=c["Lq"], his=c["Lh"], cap=c["Lc"], trg=c["Lt"], frames=c["T"]))

    def loop(tr, n):
        ops.DROP_CTR = tr.drop_ctr
        for _ in range(5):
            tr.step(bb)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            tr.step(bb)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / n
    pad = {"exact_ms": [], "class_ms": [], "unpadded_class_ms": []}
    for _ in range(3):                                                 # alternated
        pad["exact_ms"].append(loop(tr_e, a.bench_steps))
        pad["class_ms"].append(loop(tr_c, a.bench_steps))
        pad["unpadded_class_ms"].append(loop(tr_f, a.bench_steps))
    pad["class_geometry"] = lc.shape(bb)
    pad["class_over_exact"] = min(pad["class_ms"]) / min(pad["exact_ms"])
    pad["unpadded_class_over_exact"] = min(pad["unpadded_class_ms"]) / min(pad["exact_ms"])
    out["padding"] = pad
    out["stage"] = stage_rate(c, a.iters)
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
