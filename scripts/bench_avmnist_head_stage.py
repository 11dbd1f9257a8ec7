#!/usr/bin/env python
"""What the AVMNIST head stage costs per step: the fusion head trained on frozen encoders, one pattern per sample or
every pattern of the batch in one step, next to the all-trainable step it follows.

ResNet18(1, 64) + ResNet34(1, 128), hidden 128, dropout 0.5, B = 128, all three patterns, a synthetic batch.  Legs:

  train_step          ``FusedTrainStep`` at B on an all-trainable model (the step before this stage existed)
  head_stage          ``FusedHeadStageStep`` at B (frozen encoders, one random pattern per sample)
  pattern_kernel      ``FusedHeadStagePatternStep`` at B, ``head="kernel"`` (``tspm_pattern_head_train_step``)
  pattern_launches    ``FusedHeadStagePatternStep`` at B, ``head="launches"`` (expand + ``tspm_head_train_step``, n = 3B)
  head_stage_3B       ``FusedHeadStageStep`` at 3B: the replicated, masked batch the all-pattern step replaces
  head_only_kernel    the head leg of pattern_kernel alone (its own captured graph: no encoders, no log, no Adam)
  head_only_launches  the head leg of pattern_launches alone

Protocol (DESIGN §3.19's): every leg is built and warmed up (eager, capture, replay) in this one process; then ``--runs``
rounds (5), each timing the legs one after the other (interleaved): ``--replays`` replays of the leg's captured graph, one
pair of device events per replay.  A round's figure is the median of its replays, a leg's the median of its round
medians, with their range.  Nothing in the package reads the result; ``step.DEFAULT_HEAD_STAGE_HEAD`` records which head
measured lower.  Needs the MI355X: there is no CPU leg.

    python scripts/bench_avmnist_head_stage.py --out profiles/avmnist_head_stage.json
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

BATCH, PATTERNS = 128, ("a", "ai", "i")
LEGS = ("train_step", "head_stage", "pattern_kernel", "pattern_launches", "head_stage_3B", "head_only_kernel",
        "head_only_launches")


def timed_calls(fn, n):
    import torch
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)


def spread(xs):
    return {"median_us": statistics.median(xs), "min_us": min(xs), "max_us": max(xs), "round_medians_us": xs}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--replays", type=int, default=100, help="timed graph replays per leg and round")
    ap.add_argument("--warmup", type=int, default=5, help="untimed steps per leg (eager, capture, replays)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "avmnist_head_stage.json"))
    a = ap.parse_args()
    if a.warmup < 3:
        raise SystemExit("bench_avmnist_head_stage: --warmup >= 3 (the second call of a step captures its graph)")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_avmnist_head_stage: needs the MI355X (no CPU leg)")
    import tspm_amd
    from oracle import avmnist_ref as orc
    from tspm_amd import _lib as L
    from tspm_amd import step
    dev = torch.device("cuda", 0)

    def model(frozen):
        torch.manual_seed(0)
        m = tspm_amd.AVMNIST(tspm_amd.ResNet18(1, 64), tspm_amd.ResNet34(1, 128), 128, dropout=0.5).to(dev)
        return m.freeze_encoders() if frozen else m

    def batch(n, masked):
        audio, image, labels, _ = orc.synthetic_batch(n, seed=1234)
        if masked:  # one random pattern per sample, applied to the inputs
            g = torch.randint(0, 3, (n,), generator=torch.Generator().manual_seed(1))
            ka = torch.tensor([step.PATTERN_KEEP[PATTERNS[k]][0] for k in g.tolist()], dtype=torch.float32)
            ki = torch.tensor([step.PATTERN_KEEP[PATTERNS[k]][1] for k in g.tolist()], dtype=torch.float32)
            audio, image = audio * ka.view(n, 1, 1), image * ki.view(n, 1, 1, 1)
        return audio.to(dev), image.to(dev), labels.to(dev)

    full, frozen = model(False), model(True)
    opt_full = tspm_amd.FusedAdam(full.parameters(), lr=5e-4, weight_decay=1e-4)
    # the frozen model's steps share its one optimizer (built after freeze_encoders(): the head's parameters only)
    opt =tspm_amd.FusedAdam(frozen.parameters(), lr=5e-4, weight_decay=1e-4)
    steps = {"train_step": tspm_amd.FusedTrainStep(full, opt_full, None, BATCH),
             "head_stage": step.FusedHeadStageStep(frozen, opt, None, BATCH),
             "pattern_kernel": step.FusedHeadStagePatternStep(frozen, opt, None, BATCH, PATTERNS, head="kernel"),
             "pattern_launches": step.FusedHeadStagePatternStep(frozen, opt, None, BATCH, PATTERNS, head="launches"),
             "head_stage_3B": step.FusedHeadStageStep(frozen, opt, None, 3 * BATCH)}
    assert steps["pattern_kernel"].head == "kernel" and steps["pattern_launches"].head == "launches"
    data = {"train_step": batch(BATCH, True), "head_stage": batch(BATCH, True), "pattern_kernel": batch(BATCH, False),
            "pattern_launches": batch(BATCH, False), "head_stage_3B": batch(3 * BATCH, True)}
    loss = {}
    for leg, st in steps.items():
        for _ in range(a.warmup):
            out = st.step(*data[leg])
        torch.cuda.synchronize()
        loss[leg] = float(out["loss"].item())
        if st.graph is None or not torch.isfinite(out["loss"]).all():
            raise SystemExit(f"{leg}: no captured graph or a non-finite loss ({loss[leg]})")
    replay = {leg: st.graph.replay for leg, st in steps.items()}
    for head in ("kernel", "launches"):  # the head leg alone, from the embeddings the last step left in place
        st = steps["pattern_" + head]
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with L.graph_capture(g):
            st._head(torch.cuda.current_stream().cuda_stream)
        replay["head_only_" + head] = g.replay
    rounds = {leg: [] for leg in LEGS}
    for _ in range(a.runs):  # interleaved
        for leg in LEGS:
            rounds[leg].append(timed_calls(replay[leg], a.replays))
    out = {"timing": "one pair of device events per graph replay; a round = the median of its replays, a leg = the median "
                     "of its round medians; rounds interleave the legs; all legs in one process, warmed up",
           "command": "python scripts/bench_avmnist_head_stage.py --out profiles/avmnist_head_stage.json",
           "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "model": "ResNet18(1,64) + ResNet34(1,128), hidden 128, dropout 0.5", "batch": BATCH,
           "patterns": list(PATTERNS), "runs": a.runs, "replays_per_round": a.replays,
           "legs": {leg: dict(spread(rounds[leg]), **({"loss": loss[leg]} if leg in loss else {})) for leg in LEGS}}
    med = lambda leg: out["legs"][leg]["median_us"]  # noqa: E731
    out["ratios"] = {"head_stage_over_train_step": med("head_stage") / med("train_step"),
                     "pattern_kernel_over_head_stage": med("pattern_kernel") / med("head_stage"),
                     "pattern_kernel_over_head_stage_3B": med("pattern_kernel") / med("head_stage_3B"),
                     "pattern_launches_over_head_stage_3B": med("pattern_launches") / med("head_stage_3B"),
                     "pattern_kernel_over_pattern_launches": med("pattern_kernel") / med("pattern_launches"),
                     "head_only_kernel_over_head_only_launches": med("head_only_kernel") / med("head_only_launches")}
    out["head"] = {"kernel_step_us": med("pattern_kernel"), "launches_step_us": med("pattern_launches"),
                   "kernel_head_only_us": med("head_only_kernel"), "launches_head_only_us": med("head_only_launches"),
                   "lower_step_median": "kernel" if med("pattern_kernel") <= med("pattern_launches") else "launches",
                   "default": step.DEFAULT_HEAD_STAGE_HEAD}
    print({leg: round(med(leg), 1) for leg in LEGS}, out["ratios"], out["head"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
