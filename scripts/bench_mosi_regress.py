#!/usr/bin/env python
"""The graph-replayed fused train step in sentiment-regression mode (one-output head, float32 scores, L1;
``tspm_regress_head_step``) against the same model's classification step (three classes, cross-entropy:
tspm_linear_fwd, tspm_cross_entropy, tspm_classify_update, tspm_linear_bwd for ``fc_out``), both recording into
their epoch log on the device.

Cases: the MOSI UTT-Fusion step at B=128, T=50; the MOSEI step at B=256, T=50; the audio encoder pre-training step
(LSTM "last", 5-d) at B=128, T=50.  Per case both variants are built from the same seed in ONE process, warmed up
(eager, capture, replays), and timed in alternating rounds: each round is ``--replays`` back-to-back replays of the
captured step between two device events (device time per step with the queue kept full; the synthetic batch stays in
the step's input buffers).  Medians, quartiles and extremes over the rounds go to the JSON; "faster_beyond_spread" /
"slower_beyond_spread" = the median difference exceeds the larger of the two inter-quartile ranges.  No default of
the package depends on the result.  Needs the MI355X: there is no CPU leg.

    python scripts/bench_mosi_regress.py --out profiles/mosi_regress_step.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

CASES = [("mosi_fusion", "mosi", 128), ("mosei_fusion", "mosei", 256), ("audio_pretrain", "audio", 128)]


def l1_group():
    import torch.nn as nn
    return {"regression": SimpleNamespace(loss_fn=nn.L1Loss(), weight=1.0)}


def build(what, regress, batch, steps, seed):
    """→ (step with its log attached, zero-argument ``load`` that puts the synthetic batch into its buffers, the
    step's device loss scalar)."""
    import torch
    import tspm_amd
    from tspm_amd import mosi as M
    from tspm_amd.metrics import ClassificationLog, RegressionLog
    from tspm_amd.monomodal import FusedMosiMonoStep, MonomodalEncoder
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1234)
    group = l1_group() if regress else None
    torch.manual_seed(seed)
    if what == "audio":
        model = MonomodalEncoder(M.LSTMEncoder(5, 64, "last"), 64, 1 if regress else 3).to(dev)
        opt = tspm_amd.FusedAdam(model.parameters(), lr=1e-3, weight_decay=1e-3)
        log = RegressionLog(dev, ("audio",)) if regress else ClassificationLog(dev, ("audio",), classes=3)
        st = FusedMosiMonoStep(model, opt, group, (batch, steps, 5), log=log)
        x = torch.randn(batch, steps, 5, generator=g).to(dev)
        scores = (torch.randint(-15, 16, (batch,), generator=g).float() / 5).to(dev)
        y = scores if regress else (scores.sign().long() + 1)
        return st, (lambda: st.load_batch(x, y)), st.loss
    c = M.YAML_CONFIGS[what]
    model = M.build_utt_fusion(what, output_dim=1 if regress else 3).to(dev)
    opt = tspm_amd.FusedAdam(model.parameters(), lr=c["lr"], weight_decay=c["weight_decay"])
    st = M.FusedMosiStep(model, opt, group, batch, steps)
    st.log = RegressionLog(dev, list(M.PATTERNS)) if regress else ClassificationLog(dev, list(M.PATTERNS), classes=3)
    A = torch.randn(batch, steps, c["audio_dim"], generator=g).to(dev)
    V = (0.5 * torch.randn(batch, steps, c["video_dim"], generator=g)).to(dev)
    T = (0.3 * torch.randn(batch, steps, c["text_dim"], generator=g)).to(dev)
    scores = (torch.randint(-15, 16, (batch,), generator=g).float() / 5).to(dev)
    y = scores if regress else (scores.sign().long() + 1)
    return st, (lambda: st.eng.load(A, V, T, y, regress)), st.eng.loss


def summarise(us):
    q = statistics.quantiles(us, n=4)
    return {"median_us": statistics.median(us), "p25_us": q[0], "p75_us": q[2], "min_us": min(us), "max_us": max(us),
            "rounds_us": [round(v, 3) for v in us]}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--replays", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mosi_regress_step.json"))
    a = ap.parse_args()
    import math

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mosi_regress: needs the MI355X (no CPU leg)")
    result = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
              "steps": a.steps, "rounds": a.rounds, "replays_per_round": a.replays,
              "timing": "device events around back-to-back graph replays", "cases": {}}
    for name, what, batch in CASES:
        steps, losses = {}, {}
        for regress in (True, False):
            st, load, loss = build(what, regress, batch, a.steps, 3)
            load()
            for _ in range(a.warmup):  # eager, capture, replays
                st.run()
            torch.cuda.synchronize()
            if st.graph is None:
                raise SystemExit("bench_mosi_regress: the step was not captured (TSPM_NO_GRAPH set?)")
            losses[regress] = loss.item()
            if not math.isfinite(losses[regress]):
                raise SystemExit(f"{name}: non-finite loss after warm-up: {losses}")
            steps[regress] = st
        times = {True: [], False: []}
        for r in range(a.rounds):
            for regress in ((True, False) if r % 2 == 0 else (False, True)):
                st = steps[regress]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.replays):
                    st.graph.replay()
                e1.record()
                e1.synchronize()
                times[regress].append(e0.elapsed_time(e1) * 1e3 / a.replays)
        reg, cls = summarise(times[True]), summarise(times[False])
        gain = cls["median_us"] - reg["median_us"]
        spread = max(reg["p75_us"] - reg["p25_us"], cls["p75_us"] - cls["p25_us"])
        result["cases"][name] = {"batch": batch, "regression": reg, "classification": cls, "median_gain_us": gain,
                                 "spread_us": spread, "faster_beyond_spread": bool(gain > spread),
                                 "slower_beyond_spread": bool(-gain > spread),
                                 "loss_after_warmup": {"regression": losses[True], "classification": losses[False]}}
        print(f"{name} (B={batch}): regression {reg['median_us']:.2f} us [{reg['p25_us']:.2f}, {reg['p75_us']:.2f}]  "
              f"classification {cls['median_us']:.2f} us [{cls['p25_us']:.2f}, {cls['p75_us']:.2f}]  gain {gain:.2f} us "
              f"(spread {spread:.2f})", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out, "gains_us": {k: round(v["median_gain_us"], 3) for k, v in result["cases"].items()}}))


if __name__ == "__main__":
    main()
