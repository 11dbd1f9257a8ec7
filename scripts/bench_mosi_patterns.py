#!/usr/bin/env python
"""What evaluating every missing-modality pattern of a batch from one encoder pass saves: ``MosiEpochRunner.validate_epoch``
over a synthetic corpus on the per-pattern loader (each utterance encoded once per pattern: P ``FusedMosiEvalStep`` replays
per batch of utterances) next to the fused loader (``MOSI.loader(fuse_patterns=True)``: one ``FusedMosiPatternEvalStep``
replay per batch — a 2B-row encoder pass, ``tspm_pattern_expand``, the classifier on P*B rows, P loss / metrics launches).

Shapes (Ta, Tv, Tt): MOSI aligned 50 at B = 128, MOSI (375, 500, 50) at B = 128, MOSEI (500, 375, 50) at B = 256; all seven
patterns; ``--batches`` batches of utterances per epoch (the sample count is a multiple of the batch, so both loaders cut
the same batches and log the same number of loss entries).

Protocol: both legs' steps are built and warmed up (``--warmup`` epochs: eager, capture, replay) in the same process; then
``--runs`` rounds (5), each timing the legs one after the other (interleaved), ``--epochs`` epochs per leg and round, each
epoch between a pair of device events on the current stream and a host clock (the epoch ends in the log's read-back, a
device synchronise); a round's figure is the median of its epochs, a leg's the median of its round medians, with their
range.  ``batches``: the same epoch without its read-back and the host's metric functions (gathers and replays only,
device events around the loop over the batches).  ``replay``: the captured graphs alone, one pair of device events per
replay, P per-pattern replays against one fused replay.  ``same_results``: the two legs' confusion counts are compared
and the two mean losses reported.

Nothing in the package depends on the result.  Needs the MI355X: there is no CPU leg.

    python scripts/bench_mosi_patterns.py --out profiles/mosi_patterns.json
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

SHAPES = {"mosi_aligned": ("mosi", 128, 50), "mosi": ("mosi", 128, (375, 500, 50)), "mosei": ("mosei", 256, (500, 375, 50))}
LEGS = ("per_pattern", "fused")


def dense_corpus(name, n, steps, seed=1234):
    """A dense synthetic split at the YAML's feature dims, each modality at its own length."""
    import numpy as np
    from tspm_amd import mosi as M
    from tspm_amd.mosi_data import MODALITIES, MosiCorpus
    c = M.YAML_CONFIGS[name]
    g = np.random.default_rng(seed)
    feats = (c["audio_dim"], c["video_dim"], c["text_dim"])
    seqs = {m: list(g.standard_normal((n, t, f), dtype=np.float32))
            for m, t, f in zip(MODALITIES, M.steps_triple(steps), feats)}
    return MosiCorpus(seqs, g.integers(0, 3, n).astype(np.int64))


def timed_epoch(runner, loader):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    loss, _, _, entries = runner.validate_epoch(loader)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3, (time.perf_counter() - t0) * 1e6, loss, entries


def timed_batches(runner, loader):
    """The epoch's device work alone — per batch the gather launches and the replays, as ``validate_epoch`` issues them —
    without the epoch's read-back and the host's metric functions: device events around the loop."""
    import torch
    runner.log.reset()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    with torch.no_grad():
        for b in runner.loader_for(loader, False):
            for g in runner._groups(b):
                runner._run(runner._eval_step_of(g), g)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3, (time.perf_counter() - t0) * 1e6


def replay_median(st, n):
    import torch
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for e0, e1 in ev:
        e0.record()
        st.graph.replay()
        e1.record()
    torch.cuda.synchronize()
    return statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)


def time_shape(key, a):
    import numpy as np
    import torch
    import tspm_amd
    from tspm_amd import harness
    from tspm_amd import mosi as M
    from tspm_amd.mosi_data import MOSI
    name, batch, steps = SHAPES[key]
    dev = torch.device("cuda", 0)
    c = M.YAML_CONFIGS[name]
    torch.manual_seed(3)
    model = M.build_utt_fusion(name).to(dev)
    opt = tspm_amd.FusedAdam(model.parameters(), lr=c["lr"], weight_decay=c["weight_decay"])
    n = a.batches * batch
    ds = MOSI(split="valid", corpus=dense_corpus(name, n, steps), device=dev)
    # one runner per leg: each keeps its own log, so the other leg's epochs never reset what is being read
    runners = {leg: harness.MosiEpochRunner(model, opt, None) for leg in LEGS}
    loaders = {"per_pattern": ds.loader(batch), "fused": ds.loader(batch, fuse_patterns=True)}
    conf, loss = {}, {}
    for leg in LEGS:
        for _ in range(a.warmup):
            _, _, loss[leg], entries = timed_epoch(runners[leg], loaders[leg])
        conf[leg] = runners[leg].log.fetch()[0]
        if entries != 7 * a.batches or not np.isfinite(loss[leg]):
            raise SystemExit(f"{key} {leg}: {entries} loss entries (expected {7 * a.batches}), mean loss {loss[leg]}")
    rounds = {leg: {"device_us": [], "wall_us": [], "batches_us": []} for leg in LEGS}
    for _ in range(a.runs):  # interleaved
        for leg in LEGS:
            ep = [timed_epoch(runners[leg], loaders[leg])[:2] for _ in range(a.epochs)]
            rounds[leg]["device_us"].append(statistics.median(e[0] for e in ep))
            rounds[leg]["wall_us"].append(statistics.median(e[1] for e in ep))
            rounds[leg]["batches_us"].append(statistics.median(timed_batches(runners[leg], loaders[leg])[0]
                                                               for _ in range(a.epochs)))
    steps_of = {"per_pattern": runners["per_pattern"].eval_step_for(batch, steps),
                "fused": runners["fused"].pattern_eval_step_for(batch, steps)}
    replays = a.replays if isinstance(steps, int) else a.long_replays
    replay = {leg: [] for leg in LEGS}
    for _ in range(a.runs):
        for leg in LEGS:
            replay[leg].append(replay_median(steps_of[leg], replays))
    out = {"model": name, "batch": batch, "steps": list(M.steps_triple(steps)), "samples": n, "patterns": 7,
           "loss_entries_per_epoch": 7 * a.batches, "legs": {}}
    for leg in LEGS:
        d, w, bt = rounds[leg]["device_us"], rounds[leg]["wall_us"], rounds[leg]["batches_us"]
        out["legs"][leg] = {"epoch_device_median_us": statistics.median(d), "epoch_device_min_us": min(d),
                            "epoch_device_max_us": max(d), "epoch_device_round_medians_us": d,
                            "epoch_wall_median_us": statistics.median(w), "epoch_wall_min_us": min(w),
                            "epoch_wall_max_us": max(w), "batches_device_median_us": statistics.median(bt),
                            "batches_device_min_us": min(bt), "batches_device_max_us": max(bt),
                            "replays_per_batch": 7 if leg == "per_pattern" else 1,
                            "replay_median_us": statistics.median(replay[leg]), "replay_min_us": min(replay[leg]),
                            "replay_max_us": max(replay[leg]), "mean_loss": loss[leg]}
    pp, fu = out["legs"]["per_pattern"], out["legs"]["fused"]
    out["fused_over_per_pattern"] = {"epoch_device": fu["epoch_device_median_us"] / pp["epoch_device_median_us"],
                                     "epoch_wall": fu["epoch_wall_median_us"] / pp["epoch_wall_median_us"],
                                     "batches_device": fu["batches_device_median_us"] / pp["batches_device_median_us"],
                                     "replays_per_batch": fu["replay_median_us"] / (7 * pp["replay_median_us"])}
    out["same_results"] = {"confusion_counts_equal": bool(np.array_equal(conf["fused"], conf["per_pattern"])),
                           "confusion_rows_that_differ": int(np.abs(conf["fused"] - conf["per_pattern"]).sum()) // 2,
                           "mean_loss_abs_diff": abs(loss["fused"] - loss["per_pattern"])}
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, default=8, help="batches of utterances per epoch")
    ap.add_argument("--epochs", type=int, default=3, help="timed epochs per leg and round")
    ap.add_argument("--warmup", type=int, default=3, help="untimed epochs per leg (eager, capture, replay)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--replays", type=int, default=200, help="timed graph replays per leg and round at the aligned shape")
    ap.add_argument("--long-replays", type=int, default=40, help="... at the unaligned shapes")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mosi_patterns.json"))
    a = ap.parse_args()
    if a.warmup < 2:
        raise SystemExit("bench_mosi_patterns: --warmup >= 2 (the second call of a step captures its graph)")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mosi_patterns: needs the MI355X (no CPU leg)")
    result = {"timing": "validate_epoch between a pair of device events and a host clock (it ends in the log's read-back); a "
                        "round = the median of its epochs, a leg = the median of its round medians; rounds interleave the legs; "
                        "batches = that epoch's loop over the batches alone (no read-back, no host metrics); "
                        "replay = one pair of device events per graph replay",
              "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
              "runs": a.runs, "epochs_per_round": a.epochs, "shapes": {}}
    for key in [k for k in a.shapes.split(",") if k]:
        result["shapes"][key] = r = time_shape(key, a)
        print(key, {leg: (round(v["epoch_device_median_us"], 1), round(v["batches_device_median_us"], 1),
                          round(v["replay_median_us"], 1))
                    for leg, v in r["legs"].items()}, r["fused_over_per_pattern"], r["same_results"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
