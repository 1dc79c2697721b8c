"""Validation on ragged batches: the eager validation pass against Trainer.evaluate, at BASELINE configs[1] size.

The batches are scripts/bench_ragged.py's: 200 seeded AVSD-like batches, each padded to its own maxima, B=16, bf16.

  python scripts/bench_eval_ragged.py [--steps 200] [--rounds 2] [--train-steps 20] [--out profiles/eval_classes_v1.json]
      two validation passes with `train-steps` optimiser steps between them; in every pass the two paths alternate in one process, in
      `rounds` blocks each of steps / rounds batches:
        eager    model.eval(), torch.no_grad(), run_epoch(..., eval=True) with SimpleLossCompute(opt=None) on a model of its own
        classes  Trainer.evaluate (use_graph=True, length_classes=LengthClasses()) -- one forward-only captured step per class
      reported per pass and path: ms per batch (per round and overall); for `classes` also the steady-state step (median of the steps
      that hit the store), the capture step, the captures of each pass, bytes per entry; then both paths free-running (no
      synchronisation between batches), and the training class step (Trainer.step) on the same batches for scale.

Every batch is followed by a device synchronisation in the passes (so that a batch's time is its own: captures and replays alike, the
same for both paths); the free-running lines are not.
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import bench  # noqa: E402  (sets the HIP runtime switches of the split executor before the runtime starts)
from bench_ragged import ragged_batches  # noqa: E402


def timed(part, times, probe=None, flags=None):
    """Yield the batches of `part`; the time from handing one out to being asked for the next (device drained at both ends) goes to
    `times`, and whether `probe()` stayed the same meanwhile (no capture) to `flags`."""
    for bt in part:
        before = probe() if probe is not None else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        yield bt
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        if probe is not None:
            flags.append(probe() == before)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--train-steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    c = dict(bench.CFG)

    import bist_amd.model as M
    from bist_amd import functional as Fn, ops
    from bist_amd.data.classes import LengthClasses
    from bist_amd.model.label_smoothing import LabelSmoothing
    from bist_amd.model.optimize import SimpleLossCompute
    from bist_amd.train import Trainer, run_epoch
    if Fn.main_stream() is not None:
        torch.cuda.set_stream(Fn.main_stream())
    dtype = torch.bfloat16
    args = bench.model_args(c["L"], c["d"], c["h"], 0.1)
    g = torch.Generator(device="cuda").manual_seed(7)
    pool = [torch.randn(c["B"], c["T"], c["S"], c["C"], generator=g, device="cuda", dtype=torch.float32).to(dtype) for _ in range(4)]
    batches = ragged_batches(a.steps, 2024, c, dtype, pool)
    del pool

    def model():
        torch.manual_seed(1)
        return M.make_model(c["V"], c["V"], args, ft_sizes=[c["C"]]).cuda()
    lc = LengthClasses()
    m_e = model().to(dtype).eval()                      # the eager path's model (its weights stand still: only its time is of interest)
    loss_e = SimpleLossCompute(m_e.generator, m_e.ae_generator, LabelSmoothing(c["V"], 1, 0.1), opt=None, args=args)
    m_c = model()
    m_c.train()
    Fn.manual_seed(1234)
    tr = Trainer(m_c, args, c["V"], compute_dtype=dtype, use_graph=True, length_classes=lc)
    ops.DROP_CTR = tr.drop_ctr

    def eager_pass(loader):
        with torch.no_grad():
            res = run_epoch(None, loader, None, 0, m_e, loss_e, eval=True)
        return {k: float(v) for k, v in res.items()}

    def captures():
        return tr.eval_graph_stats()["captures"]
    per = a.steps // a.rounds
    passes = []
    for p in range(2):
        cap0 = captures()
        rec = {"eager_ms_per_batch_rounds": [], "classes_ms_per_batch_rounds": []}
        t_e, t_c, hit_c = [], [], []
        for r in range(a.rounds):
            part = batches[r * per:(r + 1) * per]
            n0 = len(t_e)
            res_e = eager_pass(timed(part, t_e))
            rec["eager_ms_per_batch_rounds"].append(1e3 * sum(t_e[n0:]) / len(part))
            n0 = len(t_c)
            res_c = tr.evaluate(timed(part, t_c, captures, hit_c))
            rec["classes_ms_per_batch_rounds"].append(1e3 * sum(t_c[n0:]) / len(part))
            print("pass %d round %d: eager %.2f ms, classes %.2f ms per batch; out eager %.4f classes %.4f" % (
                p, r, rec["eager_ms_per_batch_rounds"][-1], rec["classes_ms_per_batch_rounds"][-1], res_e["out"], res_c["out"]),
                file=sys.stderr, flush=True)
        hits = [t for t, h in zip(t_c, hit_c) if h]
        caps = [t for t, h in zip(t_c, hit_c) if not h]
        rec.update(eager_ms_per_batch=1e3 * sum(t_e) / len(t_e), classes_ms_per_batch=1e3 * sum(t_c) / len(t_c),
                   eager_median_ms=1e3 * float(np.median(t_e)),
                   classes_steady_ms=1e3 * float(np.median(hits)) if hits else None,
                   classes_capture_step_ms_median=1e3 * float(np.median(caps)) if caps else None,
                   captures=captures() - cap0, last_round_out={"eager": res_e["out"], "classes": res_c["out"]})
        passes.append(rec)
        if p == 0:
            for bt in batches[:a.train_steps]:
                tr.step(bt)
            torch.cuda.synchronize()
    est = tr.eval_graph_stats()
    per_entry = [e.bytes for e in tr._eval_entries.values()]

    # free-running: no synchronisation between batches (every class is captured by now), alternated twice
    free = {"eager_ms_per_batch": [], "classes_ms_per_batch": []}
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eager_pass(batches)
        free["eager_ms_per_batch"].append(1e3 * (time.perf_counter() - t0) / len(batches))
        t0 = time.perf_counter()
        tr.evaluate(batches)
        free["classes_ms_per_batch"].append(1e3 * (time.perf_counter() - t0) / len(batches))

    # for scale: the training class step on the same batches
    t_s, hit_s = [], []
    for bt in timed(batches, t_s, lambda: tr.graph_stats()["captures"], hit_s):
        tr.step(bt)
    s_hits = [t for t, h in zip(t_s, hit_s) if h]
    gst = tr.graph_stats()
    out = {
        "config": {"B": c["B"], "S": c["S"], "C": c["C"], "L": c["L"], "d": c["d"], "steps": a.steps, "rounds": a.rounds,
                   "train_steps_between_passes": a.train_steps, "dtype": "bf16", "ladder": repr(lc), "max_eval_graphs": tr.max_eval_graphs,
                   "distinct_class_keys": len({lc.key(bt) for bt in batches}),
                   "executor": "split" if any(e.split is not None for e in tr._eval_entries.values()) else "runtime"},
        "pass1": passes[0], "pass2": passes[1],
        "both_passes": {"eager_ms_per_batch": (passes[0]["eager_ms_per_batch"] + passes[1]["eager_ms_per_batch"]) / 2,
                        "classes_ms_per_batch": (passes[0]["classes_ms_per_batch"] + passes[1]["classes_ms_per_batch"]) / 2},
        "free_running": free,
        "eval_store": {"captures": est["captures"], "hits": est["hits"], "evictions": est["evictions"], "entries": est["entries"],
                       "bytes_total": est["bytes"], "bytes_per_entry": per_entry},
        "train_class_step": {"steady_ms": 1e3 * float(np.median(s_hits)) if s_hits else None, "captures": gst["captures"],
                             "evictions": gst["evictions"], "bytes_per_entry": [e.bytes for e in tr._entries.values()]},
    }
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
