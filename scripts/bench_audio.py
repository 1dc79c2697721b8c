"""What the audio modality costs -> profiles/audio_v1.json.

  python scripts/bench_audio.py [--out FILE]
      replayed training steps at BASELINE configs[1] (B = 16, T = 32, bf16, dropout 0.1, resident batch): the model without audio, with
      six audio blocks on Ta = 32, Da = 128 features, and the latter with the fusion logits as one product per part
      (autograd.FUSE_ONE_LAUNCH off, what BIST_FUSE_ONE_LAUNCH=0 selects): 3 alternating rounds of 100 steps after 5 warm-ups;
      bist_stage_audio alone at 16 x 32 x 128 and at 64 x 128 x 128; a beam-5 turn (scripts/bench_decode.py's geometry) with and
      without audio.
  python scripts/bench_audio.py --split [--out FILE]
      the step variants alone with eight hardware queues, so that the split-graph executor replays the step (four chains: the caption
      and audio layers on the fourth); stored under "split_executor".
  python scripts/bench_audio.py --stamps
      the device-side timeline (bist_amd/stamps.py) of one replayed audio step: where the audio layers sit among the chains, forward.
  python scripts/bench_audio.py --bench parent_1.json new_1.json parent_2.json new_2.json
      adds ms_per_step and executor.nodes of `bench.py --gpus 1 --steps 20 --warmup 5` result lines (files named parent* / new*).
Nothing is enforced: the numbers go into the document."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if "--split" in sys.argv and int(os.environ.get("GPU_MAX_HW_QUEUES", "0")) < 8:
    os.environ["GPU_MAX_HW_QUEUES"] = "8"     # (before the runtime starts: the split executor's four chains want hardware queues of their own)
import torch  # noqa: E402  (before bist_amd: libbist_hip.so must bind to the HIP runtime torch has loaded)
import bist_amd  # noqa: E402,F401

OUT = os.path.join(ROOT, "profiles", "audio_v1.json")
WARM, STEPS, ROUNDS = 5, 100, 3
TA, DA = 32, 128


def args_for(audio_blocks, dropout=0.1, L=None):
    import bench
    c = bench.CFG
    a = bench.model_args(c["L"] if L is None else L, c["d"], c["h"], dropout)
    a.nb_aenc_blocks = audio_blocks
    return a


def trainer_and_batch(audio: bool, one_launch: bool = True, chain: str = "auto"):
    import bench
    import bist_amd.model as M
    from bist_amd import autograd as ag, functional as Fn
    from bist_amd.model import decoder as DEC
    from bist_amd.data.synthetic import synthetic_batch
    from bist_amd.train import Trainer
    c = bench.CFG
    if Fn.main_stream() is not None:
        torch.cuda.set_stream(Fn.main_stream())
    args = args_for(c["L"] if audio else 0)
    torch.manual_seed(1)
    Fn.manual_seed(1)
    model = M.make_model(c["V"], c["V"], args, ft_sizes=[c["C"], DA] if audio else [c["C"]]).cuda()
    model.train()
    tr = Trainer(model, args, c["V"], compute_dtype=torch.bfloat16, use_graph=True)
    b = synthetic_batch(c["B"], T=c["T"], S=c["S"], C=c["C"], Lq=c["Lq"], Lh=c["Lh"], Lc=c["Lc"], Lt=c["Lt"], vocab=c["V"], seed=1234,
                        dtype=torch.bfloat16, audio=(TA, DA) if audio else None)
    ag.FUSE_ONE_LAUNCH = one_launch                    # read while the step is recorded: the warm-ups below capture it
    DEC.AUDIO_CHAIN = chain                            # (likewise)
    try:
        for _ in range(WARM):
            tr.step(b)
        torch.cuda.synchronize()
    finally:
        ag.FUSE_ONE_LAUNCH = True
        DEC.AUDIO_CHAIN = "auto"
    return tr, b


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def event_us(fn, reps=200):
    for _ in range(10):
        fn()
    res = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        res.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(res), min(res)


def stage_alone():
    from bist_amd import ops
    out = {}
    for B, Ta, PTa in ((16, 32, 32), (16, 20, 32), (64, 128, 128)):
        src = torch.randn(B, Ta, DA, device="cuda")
        dst = torch.empty(B, PTa, DA, device="cuda", dtype=torch.bfloat16)
        mask = torch.empty(B, 1, PTa, device="cuda", dtype=torch.bool)
        med, mn = event_us(lambda: ops.stage_audio(src, dst, mask))
        nbytes = src.numel() * 4 + dst.numel() * 2 + mask.numel()
        out["%dx%d->%dx%d" % (B, Ta, PTa, DA)] = {"bytes": nbytes, "us_median": round(med, 2), "us_min": round(mn, 2),
                                                    "GBps_at_median": round(nbytes / med / 1e3, 2)}
    return out


def decode_turns(audio: bool, turns=24):
    import bench
    import bist_amd.model as M
    import bist_amd.model.decode as D
    from bist_amd.data.synthetic import synthetic_batch
    c = bench.CFG
    args = args_for(c["L"] if audio else 0)
    torch.manual_seed(1)
    model = M.make_model(c["V"], c["V"], args, ft_sizes=[c["C"], DA] if audio else [c["C"]]).cuda().to(torch.bfloat16).eval()
    b1 = synthetic_batch(1, T=c["T"], S=c["S"], C=c["C"], Lq=c["Lq"], Lh=c["Lh"], Lc=c["Lc"], Lt=c["Lt"], vocab=c["V"], seed=99,
                         dtype=torch.bfloat16, audio=(TA, DA) if audio else None)
    ts = []
    before = dict(D.STATS)
    with torch.no_grad():
        for _ in range(turns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            D.beam_search_decode(model, b1, 12, 2, 0, 3, 1, beam=5, penalty=1.0, nbest=5, train_args=args)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": round(statistics.median(ts[4:]), 3), "ms_min": round(min(ts[4:]), 3),
            "device_turns": D.STATS["device"] - before["device"], "turns": turns}


def stamps():
    """One replayed audio step with timestamps: per layer, when the caption and audio layers, the decoder layer and the main chain's join
    start and end (forward), and the stream each ran on."""
    import bench
    import bist_amd.model as M
    from bist_amd import functional as Fn, stamps as S
    from bist_amd.data.synthetic import synthetic_batch
    from bist_amd.train import Trainer
    c = bench.CFG
    args = args_for(c["L"])
    torch.manual_seed(1)
    model = M.make_model(c["V"], c["V"], args, ft_sizes=[c["C"], DA]).cuda()
    model.train()
    tr = Trainer(model, args, c["V"], compute_dtype=torch.bfloat16, use_graph=True)
    b = synthetic_batch(c["B"], T=c["T"], S=c["S"], C=c["C"], Lq=c["Lq"], Lh=c["Lh"], Lc=c["Lc"], Lt=c["Lt"], vocab=c["V"], seed=1234,
                        dtype=torch.bfloat16, audio=(TA, DA))
    S.enable()
    for _ in range(5):
        tr.step(b)
    torch.cuda.synchronize()
    S.BUF.zero_()
    for _ in range(8):
        tr.step(b)
    rows = S.read()
    streams = {s: i for i, s in enumerate(sorted({s for _, s, _ in rows}))}
    keep = ("cap in f", "cap out f", "audio in f", "audio out f", "dec in f", "dec out f", "main joined", "t2s in f", "t2s ff f", "s2t in f", "s2t ff f")
    print("%10s  %-7s %s" % ("t (us)", "stream", "point"))
    for name, s, t in rows:
        if any(name.endswith(k) for k in keep):
            print("%10.1f  q%-6d %s" % (t, streams[s], name))
    per = {}
    for name, s, t in rows:
        per[name] = (t, streams[s])
    for l in range(c["L"]):
        g = lambda k: per.get("L%d %s" % (l, k), (float("nan"), -1))
        print("layer %d: caption %.0f us (q%d), audio %.0f us (q%d), both directions' chains %.0f / %.0f us, caption chain idle before the join: %.0f us"
              % (l, g("cap out f")[0] - g("cap in f")[0], g("cap in f")[1], g("audio out f")[0] - g("audio in f")[0], g("audio in f")[1],
                 g("t2s ff f")[0] - g("t2s in f")[0], g("s2t ff f")[0] - g("s2t in f")[0], g("main joined")[0] - g("audio out f")[0]))


def main():
    if "--stamps" in sys.argv:
        return stamps()
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else OUT
    doc = json.load(open(out_path)) if os.path.exists(out_path) else {}
    if "--bench" in sys.argv:
        runs = {"parent": [], "new": []}
        nodes = {"parent": [], "new": []}
        for p in sys.argv[sys.argv.index("--bench") + 1:]:
            if p.startswith("--"):
                break
            line = json.loads([ln for ln in open(p).read().splitlines() if ln.startswith("{")][-1])
            who = "parent" if os.path.basename(p).startswith("parent") else "new"
            runs[who].append(round(line["ms_per_step"], 4))
            nodes[who].append((line.get("executor") or {}).get("nodes"))
        doc["bench_py"] = {"command": "python bench.py --gpus 1 --steps 20 --warmup 5, the parent commit and this change run alternately on one MI355X",
                           "ms_per_step": runs, "executor_nodes": nodes,
                           "parent_spread": round(max(runs["parent"]) - min(runs["parent"]), 4) if runs["parent"] else None,
                           "difference_of_medians": round(statistics.median(runs["new"]) - statistics.median(runs["parent"]), 4)
                           if runs["new"] and runs["parent"] else None}
    elif "--split" in sys.argv:
        variants = {"no_audio": trainer_and_batch(False), "audio": trainer_and_batch(True), "audio_on_caption_chain": trainer_and_batch(True, chain="cap"),
                    "audio_on_main_chain": trainer_and_batch(True, chain="main")}
        rounds = []
        for _ in range(ROUNDS):
            r = {k: round(timed(lambda: t.step(b), STEPS), 4) for k, (t, b) in variants.items()}
            rounds.append(r)
            print(r, flush=True)
        doc["split_executor"] = {"step_ms_rounds": rounds, "step_ms_median": {k: statistics.median(r[k] for r in rounds) for k in rounds[0]},
                                 "executor": {k: ("split" if getattr(t, "_split", None) is not None else "runtime") for k, (t, _) in variants.items()},
                                 "GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES")}
    else:
        variants = {"no_audio": trainer_and_batch(False), "audio": trainer_and_batch(True), "audio_fusion_per_part": trainer_and_batch(True, False),
                    "audio_on_caption_chain": trainer_and_batch(True, chain="cap")}
        rounds = []
        for _ in range(ROUNDS):
            r = {k: round(timed(lambda: t.step(b), STEPS), 4) for k, (t, b) in variants.items()}
            rounds.append(r)
            print(r, flush=True)
        med = {k: statistics.median(r[k] for r in rounds) for k in rounds[0]}
        doc["what"] = ("BASELINE configs[1] geometry (B=16, T=32, bf16, dropout 0.1), replayed steps on one resident batch: the model without audio, "
                       "with six audio blocks on [16, %d, %d] features, and the same with the fusion logits as one product per part; %d alternating "
                       "rounds of %d steps after %d warm-ups, medians over the rounds (ms per step)" % (TA, DA, ROUNDS, STEPS, WARM))
        doc["device"] = torch.cuda.get_device_name(0)
        doc["step_ms_rounds"] = rounds
        doc["step_ms_median"] = med
        doc["audio_minus_no_audio_ms"] = round(med["audio"] - med["no_audio"], 4)
        doc["audio_on_caption_chain_minus_no_audio_ms"] = round(med["audio_on_caption_chain"] - med["no_audio"], 4)
        doc["fusion_per_part_minus_one_launch_ms"] = round(med["audio_fusion_per_part"] - med["audio"], 4)
        doc["executor"] = {k: ("split" if getattr(t, "_split", None) is not None else "runtime") for k, (t, _) in variants.items()}
        doc["parameters"] = {k: t.numel for k, (t, _) in variants.items()}
        del variants
        doc["stage_audio_alone"] = stage_alone()
        doc["beam5_turn"] = {"no_audio": decode_turns(False), "audio": decode_turns(True)}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
