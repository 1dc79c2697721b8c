"""What Trainer(max_grad_norm=...) costs: replayed steps at BASELINE configs[1] (B = 16, bf16, dropout 0.1, resident batch) with
max_grad_norm None / math.inf / a finite bound that clips every step, a plain trainer whose early bucket updates are switched off (so
that, where the split executor issues them, the cost splits into the lost early update and the reduction), the same three with
accumulate=True in groups of 2, and the two bist_grad_sumsq launches alone -> profiles/clip_v1.json.

  python scripts/bench_clip.py [--out FILE]                 # 3 alternating rounds of 100 steps / 50 groups per variant after 5 warm-ups
  python scripts/bench_clip.py --bench parent_1.json new_1.json parent_2.json ...
                                                            # adds ms_per_step of `bench.py --gpus 1 --steps 20 --warmup 5` result lines
                                                            # (files named parent* / new*: the parent commit and this change, run alternately on one MI355X)
The yardstick of the option's cost is this script's own `none` line on the same box; nothing is enforced."""
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before bist_amd: libbist_hip.so must bind to the HIP runtime torch has loaded, not load one of its own)
import bist_amd  # noqa: E402,F401  (sets the runtime switches of the split executor before anything initialises the device)

OUT = os.path.join(ROOT, "profiles", "clip_v1.json")
WARM, STEPS, GROUPS, K, ROUNDS = 5, 100, 50, 2, 3
SLACK = 1.03                                        # the box-to-box spread of DESIGN.md section 6b


def trainer_and_batch(early=True, **kw):
    import bench
    import bist_amd.model as M
    from bist_amd import functional as Fn
    from bist_amd.data.synthetic import synthetic_batch
    from bist_amd.train import Trainer
    c = bench.CFG
    if Fn.main_stream() is not None:
        torch.cuda.set_stream(Fn.main_stream())
    args = bench.model_args(c["L"], c["d"], c["h"], 0.1)
    torch.manual_seed(1)
    Fn.manual_seed(1)
    model = M.make_model(c["V"], c["V"], args, ft_sizes=[c["C"]]).cuda()
    model.train()
    tr = Trainer(model, args, c["V"], compute_dtype=torch.bfloat16, use_graph=True, **kw)
    if not early:
        tr.early_adam = False            # before the capture: the marks flush reductions only, the whole update runs at the tail
    b = synthetic_batch(c["B"], T=c["T"], S=c["S"], C=c["C"], Lq=c["Lq"], Lh=c["Lh"], Lc=c["Lc"], Lt=c["Lt"], vocab=c["V"], seed=1234,
                        dtype=torch.bfloat16)
    return tr, b


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def event_ms(fn, reps=30):
    for _ in range(3):
        fn()
    res = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        res.append(e0.elapsed_time(e1))
    return statistics.median(res), min(res)


def kernels_alone(tr, acc_tr):
    """The two launches of a step over their ranges (bf16 gradient: 2 bytes per element; the last pass of a group also reads 4 of acc)."""
    from bist_amd import train as T
    out = {}
    acc_tr.phase.fill_(2)
    for name, t, per in (("step", tr, 2), ("last_pass_of_a_group", acc_tr, 6)):
        for part, lo, hi, s0, ns in (("big", t.n32, t.numel, 0, T.CLIP_SLOTS_BIG), ("prefix", 0, t.n32, T.CLIP_SLOTS_BIG, T.CLIP_SLOTS_PREFIX)):
            med, mn = event_ms(lambda: t._grad_sumsq(lo, hi, s0, ns))
            nbytes = per * (hi - lo)
            out["%s_%s" % (name, part)] = {"elements": hi - lo, "slots": ns, "MB": round(nbytes / 1e6, 2), "ms_median": round(med, 4),
                                           "ms_min": round(mn, 4), "GBps": round(nbytes / med / 1e6, 1)}
        med, mn = event_ms(t._clip_hyper)
        out["%s_clip_hyper" % name] = {"slots": T.CLIP_SLOTS_BIG + T.CLIP_SLOTS_PREFIX, "ms_median": round(med, 4), "ms_min": round(mn, 4)}
    return out


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else OUT
    doc = json.load(open(out_path)) if os.path.exists(out_path) else {}
    if "--bench" in sys.argv:
        runs = {"parent": [], "new": []}
        for p in sys.argv[sys.argv.index("--bench") + 1:]:
            if p.startswith("--"):
                break
            line = [ln for ln in open(p).read().splitlines() if ln.startswith("{")][-1]
            runs["parent" if os.path.basename(p).startswith("parent") else "new"].append(round(json.loads(line)["ms_per_step"], 4))
        med = {k: statistics.median(v) for k, v in runs.items()}
        doc["bench_py_ms_per_step"] = {"command": "python bench.py --gpus 1 --steps 20 --warmup 5, parent commit and this change run alternately by one script on one MI355X",
                                       "parent": runs["parent"], "new": runs["new"], "ratio_of_medians": round(med["new"] / med["parent"], 4),
                                       "within_3_percent": med["new"] <= SLACK * med["parent"]}
    else:
        # (each trainer is built and captured before the next: a captured graph reads its own trainer's dropout counter)
        variants = {}
        tr, b = trainer_and_batch()
        for _ in range(WARM):
            tr.step(b)
        variants["none"] = tr
        tr, _ = trainer_and_batch(max_grad_norm=math.inf)
        for _ in range(WARM):
            tr.step(b)
        variants["inf"] = tr
        bound = 1e-3 * tr.clip_stats()["norm"]         # far below the norm of any later step: every step of the `finite` lines clips
        for name, kw in (("none_no_early_update", dict(early=False)), ("finite", dict(max_grad_norm=bound))):
            tr, _ = trainer_and_batch(**kw)
            for _ in range(WARM):
                tr.step(b)
            variants[name] = tr
        groups = {}
        for name, kw in (("none", {}), ("inf", dict(max_grad_norm=math.inf)), ("finite", dict(max_grad_norm=bound))):
            tr, _ = trainer_and_batch(accumulate=True, **kw)
            for _ in range(WARM):
                tr.step_group([b] * K)
            groups[name] = tr
        rounds = []
        for _ in range(ROUNDS):
            r = {"step_ms_" + k: round(timed(lambda: t.step(b), STEPS), 4) for k, t in variants.items()}
            r.update({"group_of_2_ms_" + k: round(timed(lambda: t.step_group([b] * K), GROUPS), 4) for k, t in groups.items()})
            rounds.append(r)
            print(r, flush=True)
        med = {k: statistics.median(r[k] for r in rounds) for k in rounds[0]}
        doc["what"] = ("BASELINE configs[1] geometry (B=16, T=32, bf16, dropout 0.1), replayed steps, one resident batch; Trainer.step with "
                       "max_grad_norm None / inf / a bound of 1/1000 of the norm measured after the warm-ups (every step clips), None with the "
                       "early bucket updates off, and "
                       "Trainer(accumulate=True).step_group of %d passes with the same three; %d alternating rounds of %d steps / %d groups after %d "
                       "warm-ups; medians over the rounds (ms per step, ms per group)" % (K, ROUNDS, STEPS, GROUPS, WARM))
        doc["device"] = torch.cuda.get_device_name(0)
        doc["rounds"] = rounds
        doc["median"] = med
        doc["finite_bound"] = bound
        doc["stats_after"] = {k: t.clip_stats() for k, t in list(variants.items()) + [("group_" + k, t) for k, t in groups.items()] if t.clip}
        base = med["step_ms_none"]
        doc["cost_ms_per_step"] = {"lost_early_update": round(med["step_ms_none_no_early_update"] - base, 4),
                                   "reduction_and_guard": round(med["step_ms_inf"] - med["step_ms_none_no_early_update"], 4),
                                   "inf_total": round(med["step_ms_inf"] - base, 4), "finite_total": round(med["step_ms_finite"] - base, 4),
                                   "inf_over_none": round(med["step_ms_inf"] / base, 4), "finite_over_none": round(med["step_ms_finite"] / base, 4)}
        gbase = med["group_of_2_ms_none"]
        doc["cost_ms_per_group_of_2"] = {"inf_total": round(med["group_of_2_ms_inf"] - gbase, 4), "finite_total": round(med["group_of_2_ms_finite"] - gbase, 4),
                                         "inf_over_none": round(med["group_of_2_ms_inf"] / gbase, 4),
                                         "finite_over_none": round(med["group_of_2_ms_finite"] / gbase, 4)}
        doc["executor"] = "split" if getattr(variants["inf"], "_split", None) is not None else "runtime"
        doc["early_bucket_updates"] = {k: (len(t.buckets) if t.early_adam and getattr(t, "_split", None) is not None else 0)
                                       for k, t in variants.items()}
        doc["parameters"] = variants["inf"].numel
        doc["kernels_alone"] = kernels_alone(variants["inf"], groups["inf"])
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
