#!/usr/bin/env python
"""What the AVMNIST head stage costs per step once the frozen encoders' embeddings are cached.

ResNet18(1, 64) + ResNet34(1, 128), hidden 128, dropout 0.5, B = 128, all three patterns, synthetic data.  Legs:

  head_stage              ``FusedHeadStageStep`` at B (encoders + head, one random pattern per sample): a baseline
  pattern_step            ``FusedHeadStagePatternStep`` at B, its default head (encoders + head, every pattern): a baseline
  head_only               the head leg of pattern_step alone (its own captured graph: no encoders, no log, no Adam)
  cached_every_kernel     ``FusedCachedHeadStep``, every pattern, ``head="kernel"`` (``tspm_cached_head_train_step``)
  cached_every_launches   ... ``head="launches"`` (``tspm_embed_gather`` + ``tspm_pattern_head_train_step`` + log)
  cached_sample_kernel    ``FusedCachedHeadStep``, one pattern per sample, ``head="kernel"``
  cached_sample_launches  ... ``head="launches"`` (``tspm_embed_gather`` + ``tspm_head_train_step`` + log)
  pattern_eval            ``FusedPatternEvalStep`` at B (encoders + eval head, every pattern): a baseline
  cached_eval             ``FusedCachedEvalStep`` at B, every pattern

and, wall clock: the cache fill for ``--rows`` synthetic rows (60,000: ten repeats of 6,000 distinct samples), and a train
epoch plus ``validate_epoch`` of eight batches through ``EpochRunner``, uncached (``all_patterns`` / ``fuse_patterns``
loaders) and cached (their ``ids_only`` twins).

Protocol (DESIGN §3.22's): every leg is built and warmed up (eager, capture, replay) in this one process; then ``--runs``
rounds (5), each timing the legs one after the other (interleaved): ``--replays`` replays of the leg's captured graph, one
pair of device events per replay.  A round's figure is the median of its replays, a leg's the median of its round
medians, with their range.  Nothing in the package reads the result; ``step.DEFAULT_CACHED_HEAD`` records which head
measured lower.  Needs the MI355X: there is no CPU leg.

    python scripts/bench_avmnist_embedding_cache.py --out profiles/avmnist_embedding_cache.json
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

BATCH, PATTERNS, EPOCH_BATCHES = 128, ("a", "ai", "i"), 8
LEGS = ("head_stage", "pattern_step", "head_only", "cached_every_kernel", "cached_every_launches",
        "cached_sample_kernel", "cached_sample_launches", "pattern_eval", "cached_eval")


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
    ap.add_argument("--rows", type=int, default=60000, help="rows of the cache fill")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "avmnist_embedding_cache.json"))
    a = ap.parse_args()
    if a.warmup < 3:
        raise SystemExit("bench_avmnist_embedding_cache: --warmup >= 3 (the second call of a step captures its graph)")
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_avmnist_embedding_cache: needs the MI355X (no CPU leg)")
    import tspm_amd
    from oracle import avmnist_ref as orc
    from tspm_amd import _lib as L
    from tspm_amd import step
    from tspm_amd.data import AVMNIST, AVMNISTCorpus, synthetic_corpus
    from tspm_amd.harness import EpochRunner
    dev = torch.device("cuda", 0)

    torch.manual_seed(0)
    model = tspm_amd.AVMNIST(tspm_amd.ResNet18(1, 64), tspm_amd.ResNet34(1, 128), 128, dropout=0.5).to(dev)
    model.freeze_encoders()
    opt = tspm_amd.FusedAdam(model.parameters(), lr=5e-4, weight_decay=1e-4)

    # the fill: --rows rows (repeats of 6,000 distinct synthetic samples), chunks of 256
    base = synthetic_corpus(min(6000, a.rows), 1234)
    reps = -(-a.rows // len(base))
    big = AVMNISTCorpus(np.tile(base.audio, (reps, 1, 1))[:a.rows], np.tile(base.image, (reps, 1, 1))[:a.rows],
                        np.tile(base.labels, reps)[:a.rows])
    ds = AVMNIST(None, "train", "multimodal", corpus=big, device=dev)
    cache = ds.embedding_cache(model)          # the first fill builds the chunk engines: warm-up
    fills = [cache.refresh().fill_seconds for _ in range(a.runs)]

    def batch(n, masked):
        audio, image, labels, _ = orc.synthetic_batch(n, seed=1234)
        g = torch.randint(0, 3, (n,), generator=torch.Generator().manual_seed(1))
        if masked:  # one random pattern per sample, applied to the inputs
            ka = torch.tensor([step.PATTERN_KEEP[PATTERNS[k]][0] for k in g.tolist()], dtype=torch.float32)
            ki = torch.tensor([step.PATTERN_KEEP[PATTERNS[k]][1] for k in g.tolist()], dtype=torch.float32)
            audio, image = audio * ka.view(n, 1, 1), image * ki.view(n, 1, 1, 1)
        return audio.to(dev), image.to(dev), labels.to(dev)

    ids = torch.randint(0, a.rows, (BATCH,), generator=torch.Generator().manual_seed(2)).to(dev)
    gid = torch.randint(0, 3, (BATCH,), generator=torch.Generator().manual_seed(1))
    keep = torch.tensor([step.PATTERN_KEEP[PATTERNS[k]] for k in gid.tolist()], dtype=torch.uint8).to(dev)
    gid = gid.to(torch.int32).to(dev)
    C = step.FusedCachedHeadStep
    steps = {"head_stage": step.FusedHeadStageStep(model, opt, None, BATCH),
             "pattern_step": step.FusedHeadStagePatternStep(model, opt, None, BATCH, PATTERNS),
             "cached_every_kernel": C(model, opt, None, BATCH, cache, PATTERNS, head="kernel"),
             "cached_every_launches": C(model, opt, None, BATCH, cache, PATTERNS, head="launches"),
             "cached_sample_kernel": C(model, opt, None, BATCH, cache, per_sample=True, head="kernel"),
             "cached_sample_launches": C(model, opt, None, BATCH, cache, per_sample=True, head="launches"),
             "pattern_eval": step.FusedPatternEvalStep(model, None, BATCH, None, PATTERNS),
             "cached_eval": step.FusedCachedEvalStep(model, None, BATCH, cache, None, PATTERNS)}
    for leg in ("cached_every_kernel", "cached_every_launches", "cached_sample_kernel", "cached_sample_launches"):
        assert steps[leg].head == leg.rsplit("_", 1)[1], leg
    data = {"head_stage": batch(BATCH, True), "pattern_step": batch(BATCH, False), "pattern_eval": batch(BATCH, False),
            "cached_every_kernel": (ids,), "cached_every_launches": (ids,), "cached_eval": (ids,),
            "cached_sample_kernel": (ids, keep, gid), "cached_sample_launches": (ids, keep, gid)}
    loss = {}
    for leg, st in steps.items():
        for _ in range(a.warmup):
            out = st.step(*data[leg])
        torch.cuda.synchronize()
        loss[leg] = float(out["loss"].mean().item())
        if st.graph is None or not torch.isfinite(out["loss"]).all():
            raise SystemExit(f"{leg}: no captured graph or a non-finite loss ({loss[leg]})")
    replay = {leg: st.graph.replay for leg, st in steps.items()}
    g = torch.cuda.CUDAGraph()  # the head leg alone, from the embeddings the last step left in place
    torch.cuda.synchronize()
    with L.graph_capture(g):
        steps["pattern_step"]._head(torch.cuda.current_stream().cuda_stream)
    replay["head_only"] = g.replay
    rounds = {leg: [] for leg in LEGS}
    for _ in range(a.runs):  # interleaved
        for leg in LEGS:
            rounds[leg].append(timed_calls(replay[leg], a.replays))

    # a train epoch + validate_epoch of eight batches through the runner, both ways (wall clock, after one warm-up pass)
    n_ep = EPOCH_BATCHES * BATCH
    small = AVMNISTCorpus(base.audio[:n_ep], base.image[:n_ep], base.labels[:n_ep])
    tr = AVMNIST(None, "train", "multimodal", corpus=small, device=dev)
    va = AVMNIST(None, "valid", "multimodal", corpus=small, device=dev)
    for d in (tr, va):
        d.embedding_cache(model)
    runner = EpochRunner(model, opt, None)
    epochs = {"uncached": [], "cached": []}

    def epoch(cached):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        runner.train_epoch(tr.device_loader(BATCH, shuffle=True, all_patterns=True, ids_only=cached))
        runner.validate_epoch(va.device_loader(BATCH, fuse_patterns=True, ids_only=cached))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    for r in range(a.runs + 1):  # interleaved; the first pass builds and captures the steps
        for name in ("uncached", "cached"):
            ms = epoch(name == "cached")
            if r:
                epochs[name].append(ms)

    out = {"timing": "one pair of device events per graph replay; a round = the median of its replays, a leg = the median "
                     "of its round medians; rounds interleave the legs; all legs in one process, warmed up; the fill and "
                     "the epochs are wall clock between device synchronisations",
           "command": "python scripts/bench_avmnist_embedding_cache.py --out profiles/avmnist_embedding_cache.json",
           "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "model": "ResNet18(1,64) + ResNet34(1,128), hidden 128, dropout 0.5", "batch": BATCH,
           "patterns": list(PATTERNS), "runs": a.runs, "replays_per_round": a.replays,
           "legs": {leg: dict(spread(rounds[leg]), **({"loss": loss[leg]} if leg in loss else {})) for leg in LEGS},
           "fill": dict(spread(fills, "s"), rows=a.rows, chunk=cache.chunk, bytes=cache.emb.numel() * 4,
                        distinct_rows=len(base)),
           "epoch_train_plus_validate_8_batches": {k: spread(v, "ms") for k, v in epochs.items()}}
    med = lambda leg: out["legs"][leg]["median_us"]  # noqa: E731
    share = med("pattern_step") - med("head_only")
    out["encoders_share_of_pattern_step_us"] = share
    out["saved_us"] = {"every_kernel": med("pattern_step") - med("cached_every_kernel"),
                       "every_launches": med("pattern_step") - med("cached_every_launches"),
                       "sample_kernel": med("head_stage") - med("cached_sample_kernel"),
                       "sample_launches": med("head_stage") - med("cached_sample_launches"),
                       "eval": med("pattern_eval") - med("cached_eval")}
    out["ratios"] = {"cached_every_kernel_over_pattern_step": med("cached_every_kernel") / med("pattern_step"),
                     "cached_sample_kernel_over_head_stage": med("cached_sample_kernel") / med("head_stage"),
                     "cached_every_kernel_over_launches": med("cached_every_kernel") / med("cached_every_launches"),
                     "cached_sample_kernel_over_launches": med("cached_sample_kernel") / med("cached_sample_launches"),
                     "cached_eval_over_pattern_eval": med("cached_eval") / med("pattern_eval"),
                     "epoch_cached_over_uncached": statistics.median(epochs["cached"]) /
                     statistics.median(epochs["uncached"])}
    both = med("cached_every_kernel") + med("cached_sample_kernel"), med("cached_every_launches") + med("cached_sample_launches")
    out["head"] = {"lower_median_every": "kernel" if med("cached_every_kernel") <= med("cached_every_launches") else "launches",
                   "lower_median_sample": "kernel" if med("cached_sample_kernel") <= med("cached_sample_launches") else "launches",
                   "lower_median_sum": "kernel" if both[0] <= both[1] else "launches", "default": step.DEFAULT_CACHED_HEAD}
    print({leg: round(med(leg), 1) for leg in LEGS}, out["ratios"], out["head"], out["fill"]["median_s"],
          {k: round(statistics.median(v), 2) for k, v in epochs.items()}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
