"""What Trainer(accumulate=True) costs: groups of K = 8 replayed passes at BASELINE configs[1] (B = 16, bf16, dropout 0.1, resident batch)
against 8 plain replayed steps in the same process, and bist_adam_accum_dev alone in its three phases beside a device-to-device copy of
the same byte count -> profiles/accumulate_v1.json.

  python scripts/bench_accumulate.py [--out FILE]            # 3 rounds of: 5 + 20 x 8 plain steps, then 5 + 20 groups of 8
  python scripts/bench_accumulate.py --bench parent_1.json new_1.json parent_2.json ...
                                                             # adds ms_per_step of `bench.py --gpus 1 --steps 20 --warmup 5` result lines
                                                             # (files named parent* / new*: the parent commit and this change, run alternately on one MI355X)
Conditions recorded, not enforced: a group of 8 takes at most 8 plain steps x 1.03; bench.py stays within 3 % of the parent."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before bist_amd: libbist_hip.so must bind to the HIP runtime torch has loaded, not load one of its own)
import bist_amd  # noqa: E402,F401  (sets the runtime switches of the split executor before anything initialises the device)

OUT = os.path.join(ROOT, "profiles", "accumulate_v1.json")
K, WARM, GROUPS, ROUNDS = 8, 5, 20, 3
SLACK = 1.03                                        # the box-to-box spread of DESIGN.md section 6b


def trainer_and_batch(accumulate):
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
    tr = Trainer(model, args, c["V"], compute_dtype=torch.bfloat16, use_graph=True, accumulate=accumulate)
    b = synthetic_batch(c["B"], T=c["T"], S=c["S"], C=c["C"], Lq=c["Lq"], Lh=c["Lh"], Lc=c["Lc"], Lt=c["Lt"], vocab=c["V"], seed=1234,
                        dtype=torch.bfloat16)
    return tr, b


def plain_round(tr, b):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(GROUPS * K):
        tr.step(b)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / (GROUPS * K)


def group_round(tr, b):
    """20 groups of 8: wall time per group, and HIP events around every pass's replay (recorded on the step's stream)."""
    events = []
    inner = tr._graph_open

    def timed(batch):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = inner(batch)
        e1.record()
        events.append((e0, e1))
        return out
    tr._graph_open = timed
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(GROUPS):
            tr.step_group([b] * K)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3 / GROUPS
    finally:
        tr._graph_open = inner
    ms = [e0.elapsed_time(e1) for e0, e1 in events]
    last = ms[K - 1::K]
    other = [x for i, x in enumerate(ms) if i % K != K - 1]
    return wall, statistics.mean(other), statistics.mean(last)


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


def kernel_alone(tr):
    """The launch over the whole flat range per phase (bf16 gradient and working copy), and a copy whose read + write is the same byte
    count.  Bytes per parameter, counted from the accesses: first 2 + 4, middle 2 + 4 + 4, last 2 + 4 + 3 x (4 + 4) + 2."""
    out = {}
    n = tr.numel
    for name, phase, per in (("first", 1, 6), ("middle", 0, 10), ("last", 2, 32)):
        tr.phase.fill_(phase)
        med, mn = event_ms(lambda: tr._adam_dev(0, n))
        nbytes = per * n
        half = torch.empty(nbytes // 2, device="cuda", dtype=torch.uint8)
        dst = torch.empty_like(half)
        cmed, cmn = event_ms(lambda: dst.copy_(half))
        del half, dst
        out[name] = {"bytes_per_parameter": per, "GB": round(nbytes / 1e9, 4), "ms_median": round(med, 4), "ms_min": round(mn, 4),
                     "GBps": round(nbytes / med / 1e6, 1), "copy_same_bytes_ms_median": round(cmed, 4), "copy_same_bytes_ms_min": round(cmn, 4),
                     "copy_GBps_read_plus_write": round(nbytes / cmed / 1e6, 1), "ratio_to_copy": round(med / cmed, 3)}
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
        plain, b = trainer_and_batch(False)
        for _ in range(WARM):
            plain.step(b)
        acc, _ = trainer_and_batch(True)          # (built after the plain trainer's capture: each graph reads its own trainer's dropout counter)
        for _ in range(WARM):
            acc.step_group([b] * K)
        rounds = []
        for _ in range(ROUNDS):
            p = plain_round(plain, b)
            g, other, last = group_round(acc, b)
            rounds.append({"plain_ms_per_step": round(p, 4), "group_ms": round(g, 4), "pass_ms_not_last": round(other, 4),
                           "pass_ms_last": round(last, 4)})
            print(rounds[-1], flush=True)
        med = {k: statistics.median(r[k] for r in rounds) for k in rounds[0]}
        doc["what"] = ("BASELINE configs[1] geometry (B=16, T=32, bf16, dropout 0.1), replayed steps, one resident batch; groups of K=8 passes "
                       "(Trainer(accumulate=True).step_group) against Trainer.step in the same process, %d alternating rounds of %d groups / %d steps "
                       "after %d warm-up groups / steps; medians over the rounds" % (ROUNDS, GROUPS, GROUPS * K, WARM))
        doc["device"] = torch.cuda.get_device_name(0)
        doc["K"] = K
        doc["rounds"] = rounds
        doc["median"] = med
        doc["group_over_8_plain_steps"] = round(med["group_ms"] / (K * med["plain_ms_per_step"]), 4)
        doc["group_within_8_steps_x_1.03"] = med["group_ms"] <= K * med["plain_ms_per_step"] * SLACK
        doc["executor"] = "split" if getattr(acc, "_split", None) is not None else "runtime"
        doc["early_bucket_updates"] = len(acc.buckets) if acc.early_adam and getattr(acc, "_split", None) is not None else 0
        doc["graphs"] = {"captures_of_the_accumulating_trainer": 1 if acc._graph is not None else 0,
                         "accumulator_GB": round(acc.acc.numel() * 4 / 1e9, 4), "parameters": acc.numel}
        doc["kernel_alone"] = kernel_alone(acc)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
