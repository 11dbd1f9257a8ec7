#!/usr/bin/env python
"""A/B of the MMIMDb encoder pre-training step's head: ``tspm_mono_head_bce_step`` (MonomodalEncoder(fused_head=True))
against the separate launches the library already exported (tspm_linear_fwd, tspm_bce_logits, tspm_linear_bwd;
fused_head=False), on the graph-replayed train step.

Cases: the image encoder (4096 -> 512) and the text encoder (300 -> 512) under the 23-genre classifier, at batch 128
and 256.  The protocol is scripts/bench_mosi_mono.py's: per case both variants are built from the same seed in ONE
process, warmed up (eager, capture, replays), and timed in alternating rounds: each round is ``--replays``
back-to-back replays of the captured step between two device events (device time per step with the queue kept
full; the synthetic batch stays in the step's input buffers).  Medians, quartiles and extremes over the rounds go to
the JSON; "faster_beyond_spread" = the median gain exceeds the larger of the two inter-quartile ranges — the rule
that decides, per batch size, monomodal.FUSED_BCE_HEAD_MIN_BATCH.  Needs the MI355X: there is no CPU leg.

    python scripts/bench_mmimdb_mono.py --out profiles/mmimdb_mono_head_ab.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

CASES = [("image", 4096), ("text", 300)]
EMBED, GENRES = 512, 23


def build(fin, fused_head, batch, seed, lr, wd):
    import torch
    import tspm_amd
    from tspm_amd.mmimdb import MMIMDbModalityEncoder
    from tspm_amd.monomodal import FusedMMIMDbMonoStep, MonomodalEncoder
    dev = torch.device("cuda", 0)
    torch.manual_seed(seed)
    model = MonomodalEncoder(MMIMDbModalityEncoder(fin, EMBED), EMBED, GENRES, fused_head=fused_head).to(dev)
    opt = tspm_amd.FusedAdam(model.parameters(), lr=lr, weight_decay=wd)
    st = FusedMMIMDbMonoStep(model, opt, None, (batch, fin))
    if st.fused_head is not fused_head:
        raise SystemExit("bench_mmimdb_mono: the step did not take the requested head")
    return st


def summarise(us):
    q = statistics.quantiles(us, n=4)
    return {"median_us": statistics.median(us), "p25_us": q[0], "p75_us": q[2], "min_us": min(us), "max_us": max(us),
            "rounds_us": [round(v, 3) for v in us]}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--replays", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--weight-decay", type=float, default=1e-3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mmimdb_mono_head_ab.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mmimdb_mono: needs the MI355X (no CPU leg)")
    from tspm_amd.mmimdb import synthetic_features
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
              "embed": EMBED, "genres": GENRES, "rounds": a.rounds, "replays_per_round": a.replays,
              "timing": "device events around back-to-back graph replays", "cases": {}}
    for batch in a.batches:
        image, text, labels = synthetic_features(batch, seed=1234)
        y = labels.to(dev)
        for name, fin in CASES:
            x = (image if name == "image" else text).to(dev)
            steps = {fh: build(fin, fh, batch, 3, a.lr, a.weight_decay) for fh in (True, False)}
            losses = {}
            for fh, st in steps.items():
                for _ in range(a.warmup):  # eager, capture, replays
                    st.step(x, y)
                torch.cuda.synchronize()
                if st.graph is None:
                    raise SystemExit("bench_mmimdb_mono: the step was not captured (TSPM_NO_GRAPH set?)")
                losses[fh] = st.loss.item()
            # the two variants ran the same steps from the same weights: the results must agree before the times
            # count (1 %: twenty Adam steps amplify reordered sums; tests/test_gpu_mmimdb_mono.py holds one step)
            if abs(losses[True] - losses[False]) > 1e-2 * abs(losses[False]):
                raise SystemExit(f"{name} b{batch}: losses differ after warm-up: {losses}")
            times = {True: [], False: []}
            for r in range(a.rounds):
                for fh in ((True, False) if r % 2 == 0 else (False, True)):
                    st = steps[fh]
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.replays):
                        st.graph.replay()
                    e1.record()
                    e1.synchronize()
                    times[fh].append(e0.elapsed_time(e1) * 1e3 / a.replays)
            on, off = summarise(times[True]), summarise(times[False])
            gain = off["median_us"] - on["median_us"]
            spread = max(on["p75_us"] - on["p25_us"], off["p75_us"] - off["p25_us"])
            key = f"{name}_b{batch}"
            result["cases"][key] = {"in": fin, "batch": batch, "fused_head_on": on, "fused_head_off": off,
                                    "median_gain_us": gain, "spread_us": spread,
                                    "faster_beyond_spread": bool(gain > spread),
                                    "loss_after_warmup": {"on": losses[True], "off": losses[False]}}
            print(f"{key}: fused head {on['median_us']:.2f} us [{on['p25_us']:.2f}, {on['p75_us']:.2f}]  separate "
                  f"{off['median_us']:.2f} us [{off['p25_us']:.2f}, {off['p75_us']:.2f}]  gain {gain:.2f} us "
                  f"(spread {spread:.2f})", flush=True)
    # the default is decided per batch size: the head kernel where BOTH encoders' steps are faster beyond the spread
    result["fused_head_default_by_batch"] = {
        str(b): all(c["faster_beyond_spread"] for c in result["cases"].values() if c["batch"] == b) for b in a.batches}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out, "gains_us": {k: round(v["median_gain_us"], 3) for k, v in result["cases"].items()},
                      "fused_head_default_by_batch": result["fused_head_default_by_batch"]}))


if __name__ == "__main__":
    main()
