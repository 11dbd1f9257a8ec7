#!/usr/bin/env python
"""What evaluating every missing-modality pattern of an AVMNIST batch from one encoder pass saves:
``EpochRunner.validate_epoch`` over a synthetic corpus on the default loader (each sample encoded once per pattern: three
``FusedEvalStep`` replays per batch of samples) next to the fused loader (``AVMNIST.device_loader(fuse_patterns=True)``: one
``FusedPatternEvalStep`` replay per batch — the encoders over the B real rows, the head over 3·B rows from the real rows
and the constant zero-input embeddings).

ResNet18(1, 64) + ResNet34(1, 128), hidden 128, B = 128, all three patterns; ``--batches`` batches of samples per epoch (the
sample count is a multiple of the batch, so both loaders cut single-pattern / whole batches and log the same number of
loss entries).

Protocol: every leg's steps are built and warmed up (``--warmup`` epochs: eager, capture, replay) in the same process; then
``--runs`` rounds (5), each timing the legs one after the other (interleaved).  ``epoch``: ``validate_epoch`` between a
pair of device events and a host clock (it ends in the log's read-back, a device synchronise).  ``batches``: the same
epoch's loop over the batches alone (gathers and replays; the fused leg's includes its once-per-epoch zero-embedding
refresh), device events around the loop.  ``replay``: the captured graphs alone, one pair of device events per replay,
three per-pattern replays against one fused replay, for both heads of the fused step (``kernel``: one
``tspm_pattern_head_eval`` call; ``launches``: expand + three linears + per pattern cross-entropy and classify).
``zero_refresh``: ``AVMNIST.zero_embeddings(refresh=True)`` alone (two one-row encoder forwards on two streams, eager).
A round's figure is the median of its samples, a leg's the median of its round medians, with their range.

Nothing in the package reads the result; ``step.DEFAULT_PATTERN_HEAD`` records which head measured faster.  Needs the
MI355X: there is no CPU leg.

    python scripts/bench_avmnist_patterns.py --out profiles/avmnist_patterns.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

BATCH, PATTERNS = 128, ("a", "ai", "i")
LEGS = ("per_pattern", "fused_kernel", "fused_launches")


def events():
    import torch
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed_epoch(runner, loader):
    import torch
    e0, e1 = events()
    t0 = time.perf_counter()
    e0.record()
    loss, _, _, entries = runner.validate_epoch(loader)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3, (time.perf_counter() - t0) * 1e6, loss, entries


def timed_batches(runner, loader):
    """The epoch's device work alone, as ``validate_epoch`` issues it, without the read-back and the metric functions."""
    import torch
    from tspm_amd.modules import modality_key
    runner.log.reset()
    e0, e1 = events()
    e0.record()
    fresh = False
    with torch.no_grad():
        for b in loader:
            a, i = b[modality_key(b, "audio")], b[modality_key(b, "image")]
            if b.get("fused_patterns"):
                runner.pattern_eval_step_for(a.shape[0], b["patterns"]).step(a, i, b["labels"], refresh_zero=not fresh)
                fresh = True
            else:
                runner._eval_step(a.shape[0]).step(a, i, b["labels"], b["pattern_ids"])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def timed_calls(fn, n):
    import torch
    ev = [events() for _ in range(n)]
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
    ap.add_argument("--batches", type=int, default=8, help="batches of samples per epoch")
    ap.add_argument("--epochs", type=int, default=3, help="timed epochs per leg and round")
    ap.add_argument("--warmup", type=int, default=3, help="untimed epochs per leg (eager, capture, replay)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--replays", type=int, default=100, help="timed graph replays per leg and round")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "avmnist_patterns.json"))
    a = ap.parse_args()
    if a.warmup < 2:
        raise SystemExit("bench_avmnist_patterns: --warmup >= 2 (the second call of a step captures its graph)")
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_avmnist_patterns: needs the MI355X (no CPU leg)")
    import tspm_amd
    from tspm_amd import harness, step
    from tspm_amd.data import AVMNIST, synthetic_corpus
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = tspm_amd.AVMNIST(tspm_amd.ResNet18(1, 64), tspm_amd.ResNet34(1, 128), 128, dropout=0.5).to(dev)
    n = a.batches * BATCH
    ds = AVMNIST(None, "valid", "multimodal", corpus=synthetic_corpus(n, 6), device=dev)
    # one runner per leg: each keeps its own log and its own steps
    runners = {leg: harness.EpochRunner(model, None, None) for leg in LEGS}
    loaders = {leg: ds.device_loader(BATCH, fuse_patterns=leg != "per_pattern") for leg in LEGS}
    for leg in LEGS[1:]:  # the fused legs' steps, one head each (the runner would build the default head)
        runners[leg].pattern_eval_steps[(PATTERNS, BATCH)] = step.FusedPatternEvalStep(
            model, None, BATCH, runners[leg].log, patterns=PATTERNS, head=leg.split("_")[1])
    conf, loss = {}, {}
    for leg in LEGS:
        for _ in range(a.warmup):
            _, _, loss[leg], entries = timed_epoch(runners[leg], loaders[leg])
        conf[leg] = runners[leg].log.fetch()[0]
        if entries != 3 * a.batches or not np.isfinite(loss[leg]):
            raise SystemExit(f"{leg}: {entries} loss entries (expected {3 * a.batches}), mean loss {loss[leg]}")
    steps_of = {"per_pattern": runners["per_pattern"]._eval_step(BATCH),
                **{leg: runners[leg].pattern_eval_step_for(BATCH, PATTERNS) for leg in LEGS[1:]}}
    assert steps_of["fused_kernel"].head == "kernel" and steps_of["fused_launches"].head == "launches"
    rounds = {leg: {"epoch_device": [], "epoch_wall": [], "batches_device": [], "replay": []} for leg in LEGS}
    refresh = []
    for _ in range(a.runs):  # interleaved
        for leg in LEGS:
            ep = [timed_epoch(runners[leg], loaders[leg])[:2] for _ in range(a.epochs)]
            rounds[leg]["epoch_device"].append(statistics.median(e[0] for e in ep))
            rounds[leg]["epoch_wall"].append(statistics.median(e[1] for e in ep))
            rounds[leg]["batches_device"].append(statistics.median(timed_batches(runners[leg], loaders[leg])
                                                                   for _ in range(a.epochs)))
        for leg in LEGS:
            rounds[leg]["replay"].append(timed_calls(steps_of[leg].graph.replay, a.replays))
        refresh.append(timed_calls(lambda: model.zero_embeddings(refresh=True), 20))
    out = {"timing": "epoch = validate_epoch between a pair of device events and a host clock (it ends in the log's "
                     "read-back); batches = that epoch's loop over the batches alone (no read-back, no host metrics); "
                     "replay = one pair of device events per graph replay; zero_refresh = one pair per eager refresh; a "
                     "round = the median of its samples, a leg = the median of its round medians; rounds interleave the legs",
           "command": "python scripts/bench_avmnist_patterns.py --out profiles/avmnist_patterns.json",
           "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "model": "ResNet18(1,64) + ResNet34(1,128), hidden 128", "batch": BATCH, "patterns": list(PATTERNS),
           "samples": n, "runs": a.runs, "epochs_per_round": a.epochs, "replays_per_round": a.replays,
           "loss_entries_per_epoch": 3 * a.batches, "legs": {}}
    for leg in LEGS:
        out["legs"][leg] = {"replays_per_batch": 3 if leg == "per_pattern" else 1, "mean_loss": loss[leg],
                            **{k: spread(v) for k, v in rounds[leg].items()}}
    out["zero_refresh"] = spread(refresh)
    med = lambda leg, k: out["legs"][leg][k]["median_us"]  # noqa: E731
    pp = "per_pattern"
    out["ratios"] = {leg: {"one_fused_replay_over_one_per_pattern_replay": med(leg, "replay") / med(pp, "replay"),
                           "one_fused_replay_over_three_per_pattern_replays": med(leg, "replay") / (3 * med(pp, "replay")),
                           "batches_device": med(leg, "batches_device") / med(pp, "batches_device"),
                           "epoch_device": med(leg, "epoch_device") / med(pp, "epoch_device"),
                           "epoch_wall": med(leg, "epoch_wall") / med(pp, "epoch_wall")} for leg in LEGS[1:]}
    out["head"] = {"kernel_replay_us": med("fused_kernel", "replay"), "launches_replay_us": med("fused_launches", "replay"),
                   "faster": "kernel" if med("fused_kernel", "replay") <= med("fused_launches", "replay") else "launches",
                   "default": step.DEFAULT_PATTERN_HEAD}
    out["same_results"] = {leg: {"confusion_counts_equal": bool(np.array_equal(conf[leg], conf[pp])),
                                 "confusion_rows_that_differ": int(np.abs(conf[leg] - conf[pp]).sum()) // 2,
                                 "mean_loss_rel_diff": abs(loss[leg] - loss[pp]) / abs(loss[pp])} for leg in LEGS[1:]}
    print({leg: {k: round(v["median_us"], 1) for k, v in out["legs"][leg].items() if isinstance(v, dict)} for leg in LEGS},
          "zero_refresh", round(out["zero_refresh"]["median_us"], 1), out["ratios"], out["head"], out["same_results"],
          flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
