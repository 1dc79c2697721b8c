"""What Trainer(deterministic=True) costs: the replayed training step at BASELINE configs[1] (T = 32) and at T = 128, with the mode off and
on, on the same device in one process -> profiles/deterministic_v1.json.

  python scripts/bench_deterministic.py                      # the step times (median of 5 x 20 replays each)
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_deterministic.py --trace-pass [--off]
                                                             # a run of its own for the profiler: capture + 5 replays, mode on (or off)
  python scripts/bench_deterministic.py --kernels ON_kernel_stats.csv [OFF_kernel_stats.csv]
                                                             # adds the replaced launches' rows of those summaries to the JSON
There is no pass threshold: the figure decides later whether the mode can become the default."""
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bist_amd  # noqa: E402,F401  (sets the runtime switches of the split executor before torch initialises the device)
import torch  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "deterministic_v1.json")
# the launches the mode swaps: the atomic reductions of backward.hip and their replacements of det_reduce.hip
REPLACED = ("col_sum_multi_kernel", "col_sum_kernel", "layernorm_param_grad_multi_kernel", "embed_bwd_kernel", "scaled_bias_bwd_kernel",
            "col_sum_partial_kernel", "col_sum_combine_kernel", "ln_param_partial_kernel", "ln_param_combine_kernel",
            "scaled_bias_partial_kernel", "scaled_bias_combine_kernel", "embed_bwd_det_kernel")


def trainer_and_batch(T, det):
    import bench
    import bist_amd.model as M
    from bist_amd import functional as Fn
    from bist_amd.data.synthetic import synthetic_batch
    from bist_amd.train import Trainer
    c = dict(bench.CFG, T=T)
    if Fn.main_stream() is not None:
        torch.cuda.set_stream(Fn.main_stream())
    args = bench.model_args(c["L"], c["d"], c["h"], 0.1)
    torch.manual_seed(1)
    Fn.manual_seed(1)
    model = M.make_model(c["V"], c["V"], args, ft_sizes=[c["C"]]).cuda()
    model.train()
    tr = Trainer(model, args, c["V"], compute_dtype=torch.bfloat16, use_graph=True, deterministic=det)
    b = synthetic_batch(c["B"], T=T, S=c["S"], C=c["C"], Lq=c["Lq"], Lh=c["Lh"], Lc=c["Lc"], Lt=c["Lt"], vocab=c["V"], seed=1234, dtype=torch.bfloat16)
    return tr, b


def step_ms(T, det, reps=5, steps=20):
    tr, b = trainer_and_batch(T, det)
    for _ in range(5):
        tr.step(b)
    torch.cuda.synchronize()
    res = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(steps):
            tr.step(b)
        torch.cuda.synchronize()
        res.append((time.perf_counter() - t0) * 1e3 / steps)
    del tr
    torch.cuda.empty_cache()
    return {"ms_per_step": round(statistics.median(res), 4), "runs": [round(r, 4) for r in res]}


def kernel_rows(path):
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            hit = next((k for k in REPLACED if k in name), None)
            if hit is not None:
                e = rows.setdefault(hit, {"calls": 0, "total_us": 0.0})
                e["calls"] += int(float(r.get("Calls", 0)))
                e["total_us"] += float(r.get("TotalDurationNs", 0)) / 1e3
    return {k: {"calls": v["calls"], "total_us": round(v["total_us"], 1)} for k, v in sorted(rows.items())}


def main():
    if "--trace-pass" in sys.argv:
        tr, b = trainer_and_batch(32, "--off" not in sys.argv)
        for _ in range(5):
            tr.step(b)
        torch.cuda.synchronize()
        return
    doc = json.load(open(OUT)) if os.path.exists(OUT) else {}
    if "--kernels" in sys.argv:
        paths = sys.argv[sys.argv.index("--kernels") + 1:]
        doc["kernel_stats_capture_plus_5_replays"] = {"deterministic": kernel_rows(paths[0])}
        if len(paths) > 1:
            doc["kernel_stats_capture_plus_5_replays"]["default"] = kernel_rows(paths[1])
    else:
        doc["what"] = "replayed training step, BASELINE configs[1] geometry (B=16, bf16, dropout 0.1), Trainer(deterministic=False / True)"
        doc["device"] = torch.cuda.get_device_name(0)
        for T in (32, 128):
            off, on = step_ms(T, False), step_ms(T, True)
            doc["T%d" % T] = {"default": off, "deterministic": on, "ratio": round(on["ms_per_step"] / off["ms_per_step"], 4)}
            print("T=%d: default %.3f ms/step, deterministic %.3f ms/step (x%.4f)" % (T, off["ms_per_step"], on["ms_per_step"],
                                                                                   on["ms_per_step"] / off["ms_per_step"]), flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
