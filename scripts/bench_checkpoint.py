"""What a Trainer checkpoint costs at the trainer of BASELINE configs[1] (bf16): the snapshot, restore and digest-only launches of
bist_state_copy against the device-to-device copy_ calls of the same buffers, and the wall time of save() split into the device-to-host
copy and torch.save -> profiles/checkpoint_v1.json.

  python scripts/bench_checkpoint.py [--out FILE]

HIP events on the launch stream, 5 warm-ups and 20 repeats of every variant, the variants taken in turn within each repeat (so that a
neighbour's load falls on all of them alike); medians.  Recorded, not gated: the launches run once per epoch."""
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before bist_amd: libbist_hip.so must bind to the HIP runtime torch has loaded, not load one of its own)
import bist_amd  # noqa: E402,F401  (sets the runtime switches of the split executor before anything initialises the device)

OUT = os.path.join(ROOT, "profiles", "checkpoint_v1.json")
WARM, REPS, SAVES = 5, 20, 3


def trainer_and_batch():
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
    tr = Trainer(model, args, c["V"], compute_dtype=torch.bfloat16)
    b = synthetic_batch(c["B"], T=c["T"], S=c["S"], C=c["C"], Lq=c["Lq"], Lh=c["Lh"], Lc=c["Lc"], Lt=c["Lt"], vocab=c["V"], seed=1234,
                        dtype=torch.bfloat16)
    return tr, b


def event_ms(variants):
    """name -> [ms] over REPS repeats after WARM warm-ups, the variants in turn within every repeat."""
    for fn in variants.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    res = {k: [] for k in variants}
    for _ in range(REPS):
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            res[k].append(e0.elapsed_time(e1))
    return res


def main():
    from bist_amd import checkpoint as CK
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else OUT
    tr, b = trainer_and_batch()
    for _ in range(2):                     # moments and weights of a trainer that has trained
        tr.step(b)
    torch.cuda.synchronize()
    n = tr.numel
    snap = tr.snapshot()
    live, kept = (tr.master, tr.m, tr.v), snap.tensors()
    scratch = tr._state_digests()

    def copies_out():
        for d, s in zip(kept, live):
            d.copy_(s)

    def copies_back():
        for d, s in zip(live, kept):
            d.copy_(s)
        tr.flat_param.copy_(tr.master)
    variants = {
        "snapshot_launch": lambda: CK.state_copy(live, kept, None, snap.digests),
        "three_copies": copies_out,
        "restore_launch": lambda: CK.state_copy(kept, live, tr.flat_param, scratch),
        "three_copies_and_cast": copies_back,
        "digest_only_launch": lambda: CK.state_copy(live, None, None, scratch),
    }
    nbytes = {"snapshot_launch": 24 * n, "three_copies": 24 * n, "restore_launch": 26 * n, "three_copies_and_cast": 30 * n,
              "digest_only_launch": 12 * n}             # read + written (the copy_ of the cast reads master once more)
    res = event_ms(variants)
    launches = {}
    for k, v in res.items():
        med = statistics.median(v)
        launches[k] = {"ms_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "MB": round(nbytes[k] / 1e6, 2),
                       "GBps": round(nbytes[k] / med / 1e6, 1)}
    d2h, write, size = [], [], 0
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "trainer.pt")
        for _ in range(SAVES):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sd = tr.state_dict()           # the snapshot launch, then the device-to-host copies (synchronous)
            t1 = time.perf_counter()
            torch.save(sd, path + ".tmp")
            os.replace(path + ".tmp", path)
            t2 = time.perf_counter()
            d2h.append((t1 - t0) * 1e3)
            write.append((t2 - t1) * 1e3)
            size = os.path.getsize(path)
    doc = {"what": ("Trainer of BASELINE configs[1] (bf16) after two eager steps: bist_state_copy as snapshot (live -> snapshot buffers), restore "
                    "(snapshot -> live, flat_param refreshed) and digest only, against three device-to-device copy_ calls of the same buffers "
                    "(the restore's comparison adds flat_param.copy_(master)); HIP events on the launch stream, %d warm-ups, %d repeats, variants "
                    "in turn within a repeat; save(): wall time of state_dict() (snapshot + device-to-host) and of torch.save + os.replace into "
                    "a temporary directory, %d times" % (WARM, REPS, SAVES)),
           "device": torch.cuda.get_device_name(0), "numel": n, "slots": CK.SLOTS, "launches": launches,
           "ratio_snapshot_over_copies": round(launches["snapshot_launch"]["ms_median"] / launches["three_copies"]["ms_median"], 4),
           "ratio_restore_over_copies_and_cast": round(launches["restore_launch"]["ms_median"] / launches["three_copies_and_cast"]["ms_median"], 4),
           "ratio_digest_over_snapshot": round(launches["digest_only_launch"]["ms_median"] / launches["snapshot_launch"]["ms_median"], 4),
           "save": {"file_MB": round(size / 1e6, 2), "device_to_host_ms": [round(x, 1) for x in d2h], "torch_save_ms": [round(x, 1) for x in write],
                    "device_to_host_ms_median": round(statistics.median(d2h), 1), "torch_save_ms_median": round(statistics.median(write), 1)}}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
