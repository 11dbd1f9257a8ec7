#!/usr/bin/env python
"""A/B of the MOSI encoder pre-training step's head: ``tspm_mono_head_step`` (MonomodalEncoder(fused_head=True))
against the four separate launches (tspm_linear_fwd, tspm_cross_entropy, tspm_classify_update_ex, tspm_linear_bwd;
fused_head=False), on the graph-replayed train step at B=128, T=50.

Cases: audio LSTM "last" (5-d), video LSTM "maxpool" (35-d), TextCNN (768-d).  Per case both variants are built
from the same seed in ONE process, warmed up (eager, capture, replays), and timed in alternating rounds: each
round is ``--replays`` back-to-back replays of the captured step between two device events (device time per
step with the queue kept full; the synthetic batch stays in the step's input buffers).  Medians, quartiles and
extremes over the rounds go to the JSON; "faster_beyond_spread" = the median gain exceeds the larger of the two
inter-quartile ranges.  Needs the MI355X: there is no CPU leg.

    python scripts/bench_mosi_mono.py --out profiles/mosi_mono_head_ab.json
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

CASES = [("audio_lstm_last", "lstm", 5, "last", 1.0), ("video_lstm_maxpool", "lstm", 35, "maxpool", 0.5),
         ("textcnn", "text", 768, None, 0.3)]


def build(kind, feat, embd, fused_head, batch, steps, seed, lr, wd):
    import torch
    import tspm_amd
    from tspm_amd import mosi as M
    from tspm_amd.monomodal import FusedMosiMonoStep, MonomodalEncoder
    dev = torch.device("cuda", 0)
    torch.manual_seed(seed)
    enc = M.LSTMEncoder(feat, 64, embd) if kind == "lstm" else M.TextCNN(feat, 64, dropout=0.5)
    model = MonomodalEncoder(enc, 64, 3, fused_head=fused_head).to(dev)
    opt = tspm_amd.FusedAdam(model.parameters(), lr=lr, weight_decay=wd)
    return FusedMosiMonoStep(model, opt, None, (batch, steps, feat))


def summarise(us):
    q = statistics.quantiles(us, n=4)
    return {"median_us": statistics.median(us), "p25_us": q[0], "p75_us": q[2], "min_us": min(us), "max_us": max(us),
            "rounds_us": [round(v, 3) for v in us]}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--replays", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--weight-decay", type=float, default=1e-3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mosi_mono_head_ab.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mosi_mono: needs the MI355X (no CPU leg)")
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
              "batch": a.batch, "steps": a.steps, "rounds": a.rounds,
              "replays_per_round": a.replays, "timing": "device events around back-to-back graph replays", "cases": {}}
    for name, kind, feat, embd, scale in CASES:
        g = torch.Generator().manual_seed(1234)
        x = (scale * torch.randn(a.batch, a.steps, feat, generator=g)).to(dev)
        y = torch.randint(0, 3, (a.batch,), generator=g).to(dev)
        steps = {fh: build(kind, feat, embd, fh, a.batch, a.steps, 3, a.lr, a.weight_decay) for fh in (True, False)}
        losses = {}
        for fh, st in steps.items():
            for _ in range(a.warmup):  # eager, capture, replays
                st.step(x, y)
            torch.cuda.synchronize()
            if st.graph is None:
                raise SystemExit("bench_mosi_mono: the step was not captured (TSPM_NO_GRAPH set?)")
            losses[fh] = st.loss.item()
        # the two variants ran the same steps from the same weights: the results must agree before the times count
        # (1 %: twenty Adam steps amplify reordered sums; tests/test_gpu_mosi_mono.py holds one step to 1e-6)
        if abs(losses[True] - losses[False]) > 1e-2 * abs(losses[False]):
            raise SystemExit(f"{name}: losses differ after warm-up: {losses}")
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
        result["cases"][name] = {"fused_head_on": on, "fused_head_off": off, "median_gain_us": gain,
                                 "spread_us": spread, "faster_beyond_spread": bool(gain > spread),
                                 "loss_after_warmup": {"on": losses[True], "off": losses[False]}}
        print(f"{name}: fused head {on['median_us']:.2f} us [{on['p25_us']:.2f}, {on['p75_us']:.2f}]  separate "
              f"{off['median_us']:.2f} us [{off['p25_us']:.2f}, {off['p75_us']:.2f}]  gain {gain:.2f} us "
              f"(spread {spread:.2f})", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out, "gains_us": {k: round(v["median_gain_us"], 3) for k, v in result["cases"].items()}}))


if __name__ == "__main__":
    main()
