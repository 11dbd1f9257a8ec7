#!/usr/bin/env python
"""What a cached AVMNIST head-stage epoch costs once several steps run per host call.

ResNet18(1, 64) + ResNet34(1, 128), hidden 128, dropout 0.5, B = 128, synthetic data; every pattern of the batch
("every") and one pattern per sample ("sample").  Legs, per mode:

  single          ``FusedCachedHeadStep(steps=1)``: ``tspm_cached_head_train_step`` + ``tspm_adam_step``, one replay per step
  fused_K         ``FusedCachedHeadStep(steps=K)``: one ``tspm_cached_head_train_steps`` graph of K steps (two launches a
                  step, Adam in the second), K = 8, 16, 32, 64; the figure is the replay divided by K
  separate_K      bench only: one graph of K x (``tspm_cached_head_train_step`` + ``tspm_adam_step``), the single step's
                  launches enqueued K times — what batching the replays gains without Adam in the epilogue

and, wall clock between device synchronisations: a train epoch over ``--rows`` cached rows (60,000: repeats of 6,000
distinct samples, 469 batches; every pattern and per sample) and a validation epoch over ``--val-rows`` (10,000; fused
patterns) through ``EpochRunner``, per batch and with ``steps_per_call=K``.

Protocol (DESIGN §3.23's): every leg is built and warmed up (eager, capture, replay) in this one process; then ``--runs``
rounds (5), each timing the legs one after the other (interleaved): ``--replays`` replays of the leg's captured graph, one
pair of device events per replay.  A round's figure is the median of its replays, a leg's the median of its round
medians, with their range.  The recommended ``steps_per_call`` is the smallest K whose epoch median lies within the
[min, max] of the best K's rounds.  Nothing in the package reads the result.  Needs the MI355X: there is no CPU leg.

    python scripts/bench_avmnist_cached_epoch.py --out profiles/avmnist_cached_epoch.json
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

BATCH, PATTERNS, KS = 128, ("a", "ai", "i"), (8, 16, 32, 64)


def timed_calls(fn, n):
    import torch
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)


def spread(xs, unit="us"):
    return {f"median_{unit}": statistics.median(xs), f"min_{unit}": min(xs), f"max_{unit}": max(xs),
            f"round_medians_{unit}": xs}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--replays", type=int, default=100, help="timed graph replays per leg and round")
    ap.add_argument("--warmup", type=int, default=5, help="untimed steps per leg (eager, capture, replays)")
    ap.add_argument("--rows", type=int, default=60000, help="rows of the train epoch")
    ap.add_argument("--val-rows", type=int, default=10000, help="rows of the validation epoch")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "avmnist_cached_epoch.json"))
    a = ap.parse_args()
    if a.warmup < 3:
        raise SystemExit("bench_avmnist_cached_epoch: --warmup >= 3 (the second call of a step captures its graph)")
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_avmnist_cached_epoch: needs the MI355X (no CPU leg)")
    import tspm_amd
    from tspm_amd import _lib as L
    from tspm_amd import step
    from tspm_amd.data import AVMNIST, AVMNISTCorpus, synthetic_corpus
    from tspm_amd.harness import EpochRunner
    dev = torch.device("cuda", 0)

    torch.manual_seed(0)
    model = tspm_amd.AVMNIST(tspm_amd.ResNet18(1, 64), tspm_amd.ResNet34(1, 128), 128, dropout=0.5).to(dev)
    model.freeze_encoders()
    opt = tspm_amd.FusedAdam(model.parameters(), lr=5e-4, weight_decay=1e-4)

    base = synthetic_corpus(min(6000, a.rows), 1234)

    def corpus(rows):
        reps = -(-rows // len(base))
        return AVMNISTCorpus(np.tile(base.audio, (reps, 1, 1))[:rows], np.tile(base.image, (reps, 1, 1))[:rows],
                             np.tile(base.labels, reps)[:rows])
    tr = AVMNIST(None, "train", "multimodal", corpus=corpus(a.rows), device=dev)
    va = AVMNIST(None, "valid", "multimodal", corpus=corpus(a.val_rows), device=dev)
    cache = tr.embedding_cache(model)
    va.embedding_cache(model)

    # ---- us per step ------------------------------------------------------------------------------------------------
    C = step.FusedCachedHeadStep
    kmax = max(KS)
    ids = torch.randint(0, a.rows, (kmax * BATCH,), generator=torch.Generator().manual_seed(2)).to(dev)
    gid = torch.randint(0, 3, (kmax * BATCH,), generator=torch.Generator().manual_seed(1))
    keep = torch.tensor([step.PATTERN_KEEP[PATTERNS[k]] for k in gid.tolist()], dtype=torch.uint8).to(dev)
    gid = gid.to(torch.int32).to(dev)
    replay, per_step, loss = {}, {}, {}
    for mode in ("every", "sample"):
        kw = dict(per_sample=True) if mode == "sample" else dict(patterns=PATTERNS)

        def args(k):
            n = k * BATCH
            return (ids[:n], keep[:n], gid[:n]) if mode == "sample" else (ids[:n],)
        for k in (1,) + KS:
            st = C(model, opt, None, BATCH, cache, head="kernel", steps=k, **kw)
            for _ in range(a.warmup):
                out = st.step(*args(k))
            torch.cuda.synchronize()
            leg = f"{mode}_single" if k == 1 else f"{mode}_fused_{k}"
            if st.graph is None or not torch.isfinite(out["loss"]).all():
                raise SystemExit(f"{leg}: no captured graph or a non-finite loss")
            replay[leg], per_step[leg], loss[leg] = st.graph.replay, k, float(out["loss"].item())
            if k == 1:
                single = st
        for k in KS:  # the single step's launches, K times in one graph
            g = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with L.graph_capture(g):
                for _ in range(k):
                    single._enqueue()
            leg = f"{mode}_separate_{k}"
            replay[leg], per_step[leg] = g.replay, k
            g.replay()
    torch.cuda.synchronize()
    legs = list(replay)
    rounds = {leg: [] for leg in legs}
    for _ in range(a.runs):  # interleaved
        for leg in legs:
            n = a.replays if per_step[leg] == 1 else max(10, a.replays // 4)
            rounds[leg].append(timed_calls(replay[leg], n) / per_step[leg])

    print({leg: round(statistics.median(v), 1) for leg, v in rounds.items()}, flush=True)

    # ---- epochs -----------------------------------------------------------------------------------------------------
    runner = EpochRunner(model, opt, None)
    loaders = {"train_every": lambda: tr.device_loader(BATCH, shuffle=True, all_patterns=True, ids_only=True),
               "train_sample": lambda: tr.device_loader(BATCH, shuffle=True, ids_only=True),
               "validate_fused": lambda: va.device_loader(BATCH, fuse_patterns=True, ids_only=True)}
    settings = (None,) + KS
    epochs = {name: {str(k): [] for k in settings} for name in loaders}
    batches = {}

    def epoch(name, k):
        run = runner.validate_epoch if name.startswith("validate") else runner.train_epoch
        ld = loaders[name]()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = (run(ld) if k is None else run(ld, steps_per_call=k))[3]
        torch.cuda.synchronize()
        batches[name] = n
        return (time.perf_counter() - t0) * 1e3
    for r in range(a.runs + 1):  # interleaved; the first pass builds and captures the steps
        for name in loaders:
            for k in settings:
                ms = epoch(name, k)
                if r:
                    epochs[name][str(k)].append(ms)

    out = {"timing": "one pair of device events per graph replay, divided by the steps in the graph; a round = the median "
                     "of its replays, a leg = the median of its round medians; rounds interleave the legs; all legs in one "
                     "process, warmed up; the epochs are wall clock between device synchronisations (log fetch included)",
           "command": "python scripts/bench_avmnist_cached_epoch.py --out profiles/avmnist_cached_epoch.json",
           "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "model": "ResNet18(1,64) + ResNet34(1,128), hidden 128, dropout 0.5", "batch": BATCH,
           "patterns": list(PATTERNS), "runs": a.runs, "replays_per_round": a.replays, "rows": a.rows,
           "val_rows": a.val_rows,
           "us_per_step": {leg: dict(spread(rounds[leg]), steps_per_graph=per_step[leg],
                                     **({"loss": loss[leg]} if leg in loss else {})) for leg in legs},
           "epoch_ms": {name: dict({k: spread(v, "ms") for k, v in per.items()}, batches=batches[name])
                        for name, per in epochs.items()}}
    rec = {}
    for name, per in epochs.items():
        med = {k: statistics.median(v) for k, v in per.items() if k != "None"}
        best = min(med, key=med.get)
        hi = max(per[best])
        rec[name] = {"best": int(best), "recommended": min(int(k) for k, m in med.items() if m <= hi),
                     "per_batch_over_best": statistics.median(per["None"]) / med[best]}
    out["steps_per_call"] = dict(rec, recommended=max(v["recommended"] for v in rec.values()))
    m = lambda leg: out["us_per_step"][leg]["median_us"]  # noqa: E731
    out["fused_over_separate"] = {f"{mode}_{k}": m(f"{mode}_fused_{k}") / m(f"{mode}_separate_{k}")
                                  for mode in ("every", "sample") for k in KS}
    print({leg: round(m(leg), 1) for leg in legs}, flush=True)
    print({name: {k: round(statistics.median(v), 1) for k, v in per.items()} for name, per in epochs.items()},
          out["steps_per_call"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
