#!/usr/bin/env python
"""What evaluating every missing-modality pattern of an MMIMDb batch from one encoder pass saves: one epoch's validation
of ``fit_mmimdb`` over a synthetic corpus of MM-IMDb's dev-split size (2608 samples), the default way
(``validation_loss`` over the shuffled 3·N pattern rows, then ``_evaluate`` once per pattern: every sample through the
encoders six times, eager launches) next to ``evaluate_patterns`` (each sample gathered once; one
``FusedMMIMDbPatternEvalStep`` replay per batch — the encoders and projections over the B real rows, fusion, classifier
and loss over 3·B rows), for both fusion legs (``kernel``: ``tspm_gmu_pattern_fwd`` + ``tspm_bce_logits_patterns``;
``launches``: ``tspm_pattern_expand`` + ``tspm_gmu_fwd`` + per pattern ``tspm_bce_logits``).

The GMU model of BASELINE configs[3] (4096 / 300 -> 512, hidden 512, 23 genres), all three patterns, B = 256 (BASELINE's
batch) and B = 128.

Protocol: every leg is warmed up (``--warmup`` evaluations: eager, capture, replay) in the same process; then ``--runs``
rounds (5), each timing the legs one after the other (interleaved).  ``evaluation``: the whole call between a pair of
device events and a host clock (each ends in its read-back, a device synchronise).  ``replay``: the fused step's captured
graph alone at batch B, one pair of device events per replay; for the default path the same pair around one eager
eval forward + loss of a B-row batch (one of the 6·N/B it runs).  ``zero_refresh``: ``MMIMDb.zero_projections(refresh=True)``
alone (a one-row encoder + projection pass, eager).  A round's figure is the median of its samples, a leg's the median of
its round medians, with their range.

The three legs' results are compared inside: the two fused legs must agree exactly, and every pattern's loss and F1
figures must match the default path's within the test suite's slacks (1e-4 relative, 2e-2), else the script fails.
Nothing in the package reads the result; ``mmimdb.DEFAULT_PATTERN_FUSION`` records which leg measured faster at B = 256.
Needs the MI355X: there is no CPU leg.

    python scripts/bench_mmimdb_patterns.py --out profiles/mmimdb_patterns.json
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

SAMPLES, BATCHES, PATTERNS = 2608, (256, 128), ("it", "i", "t")
LEGS = ("per_pattern", "fused_kernel", "fused_launches")


def events():
    import torch
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(fn):
    """(device us, wall us, result) of one call that ends in a device synchronise."""
    import torch
    e0, e1 = events()
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3, (time.perf_counter() - t0) * 1e6, out


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


def build_model(dev):
    import torch
    from tspm_amd import mmimdb as M
    torch.manual_seed(0)
    model = M.MMIMDb(M.MMIMDbModalityEncoder(4096, 512), M.MMIMDbModalityEncoder(300, 512),
                     gated_bimodal_network=M.GatedBiModalNetwork(input_one_dim=512, output_one_dim=512,
                                                                 input_two_dim=512, output_two_dim=512),
                     classifier=M.MLPGenreClassifier(input_size=512, hidden_size=512, output_size=23))
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():  # statistics a trained model would carry (a fresh model's zero row is the biases alone)
        for mod in model.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                c = mod.num_features
                mod.running_mean.copy_(torch.randn(c, generator=g) * 0.3)
                mod.running_var.copy_(torch.rand(c, generator=g) + 0.5)
    return model.to(dev)


def bench_batch(model, corpus, B, a):
    import torch
    from tspm_amd import _lib as L
    from tspm_amd import mmimdb as M
    vgen = torch.Generator().manual_seed(1)

    def per_pattern():
        out = {"val_loss": M.validation_loss(model, corpus, B, 1.0, PATTERNS, vgen)}
        for p in PATTERNS:
            out[p] = M._evaluate(model, corpus, B, 1.0, p)
        return out
    run = {"per_pattern": per_pattern,
           "fused_kernel": lambda: M.evaluate_patterns(model, corpus, B, fusion="kernel"),
           "fused_launches": lambda: M.evaluate_patterns(model, corpus, B, fusion="launches")}
    res = {}
    for leg in LEGS:
        for _ in range(a.warmup):
            res[leg] = run[leg]()
    steps = {leg: model.pattern_eval_step_for(None, B, PATTERNS, leg.split("_")[1]) for leg in LEGS[1:]}
    for leg, st in steps.items():
        if st.fusion != leg.split("_")[1] or st.graph is None:
            raise SystemExit(f"{leg}: built the {st.fusion} leg, graph {st.graph}")
    eng, sh = model._engine(B, corpus.device), L.stream_handle()

    def eager_batch():
        eng.forward(sh, False)
        eng.loss_fn(sh, 1.0, False, True)
    rounds = {leg: {"evaluation_device": [], "evaluation_wall": [], "replay": []} for leg in LEGS}
    refresh = []
    for _ in range(a.runs):  # interleaved
        for leg in LEGS:
            ev = [timed(run[leg])[:2] for _ in range(a.evaluations)]
            rounds[leg]["evaluation_device"].append(statistics.median(e[0] for e in ev))
            rounds[leg]["evaluation_wall"].append(statistics.median(e[1] for e in ev))
        rounds["per_pattern"]["replay"].append(timed_calls(eager_batch, a.replays))
        for leg in LEGS[1:]:
            rounds[leg]["replay"].append(timed_calls(steps[leg].graph.replay, a.replays))
        refresh.append(timed_calls(lambda: model.zero_projections(refresh=True), 20))
    # the legs' results against each other
    if res["fused_kernel"] != res["fused_launches"]:
        raise SystemExit(f"B={B}: the two fused legs disagree: {res['fused_kernel']} vs {res['fused_launches']}")
    same = {}
    for leg in LEGS[1:]:
        worst_loss = max(abs(res[leg][p]["loss"] - res["per_pattern"][p]["loss"]) / abs(res["per_pattern"][p]["loss"])
                         for p in PATTERNS)
        worst_f1 = max(abs(res[leg][p][k] - res["per_pattern"][p][k]) for p in PATTERNS
                       for k in ("f1_samples", "f1_macro", "f1_weighted", "f1_micro"))
        if worst_loss > 1e-4 or worst_f1 > 2e-2:
            raise SystemExit(f"B={B} {leg}: pattern loss rel diff {worst_loss:.2e}, F1 diff {worst_f1:.2e}")
        same[leg] = {"pattern_loss_worst_rel_diff": worst_loss, "f1_worst_abs_diff": worst_f1,
                     "val_loss_rel_diff": abs(res[leg]["val_loss"] - res["per_pattern"]["val_loss"])
                     / abs(res["per_pattern"]["val_loss"]),
                     "val_loss_note": "the default path's mean is over shuffled batches of mixed patterns, the fused "
                                      "one over per-pattern batches: equal when the batch divides the corpus, which "
                                      "2608 is not"}
    out = {"batch": B, "batches_per_evaluation": {"per_pattern": 2 * -(-3 * SAMPLES // B), "fused": -(-SAMPLES // B)},
           "legs": {leg: {"val_loss": res[leg]["val_loss"], **{k: spread(v) for k, v in rounds[leg].items()}}
                    for leg in LEGS},
           "zero_refresh": spread(refresh), "same_results": same, "fused_legs_equal": True}
    med = lambda leg, k: out["legs"][leg][k]["median_us"]  # noqa: E731
    pp = "per_pattern"
    out["ratios"] = {leg: {"evaluation_device": med(leg, "evaluation_device") / med(pp, "evaluation_device"),
                           "evaluation_wall": med(leg, "evaluation_wall") / med(pp, "evaluation_wall"),
                           "one_fused_replay_over_one_eager_batch": med(leg, "replay") / med(pp, "replay"),
                           "one_fused_replay_over_six_eager_batches": med(leg, "replay") / (6 * med(pp, "replay"))}
                     for leg in LEGS[1:]}
    out["fusion"] = {"kernel_replay_us": med("fused_kernel", "replay"), "launches_replay_us": med("fused_launches", "replay"),
                     "kernel_evaluation_us": med("fused_kernel", "evaluation_device"),
                     "launches_evaluation_us": med("fused_launches", "evaluation_device"),
                     "faster": "kernel" if med("fused_kernel", "evaluation_device") <= med("fused_launches", "evaluation_device")
                     else "launches"}
    print(B, {leg: {k: round(v["median_us"], 1) for k, v in out["legs"][leg].items() if isinstance(v, dict)} for leg in LEGS},
          "zero_refresh", round(out["zero_refresh"]["median_us"], 1), out["ratios"], out["fusion"], same, flush=True)
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--evaluations", type=int, default=3, help="timed evaluations per leg and round")
    ap.add_argument("--warmup", type=int, default=3, help="untimed evaluations per leg (eager, capture, replay)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--replays", type=int, default=100, help="timed graph replays / eager batches per leg and round")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mmimdb_patterns.json"))
    a = ap.parse_args()
    if a.warmup < 2:
        raise SystemExit("bench_mmimdb_patterns: --warmup >= 2 (the second call of a step captures its graph)")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mmimdb_patterns: needs the MI355X (no CPU leg)")
    import tspm_amd  # noqa: F401
    from tspm_amd import mmimdb as M
    dev = torch.device("cuda", 0)
    model = build_model(dev)
    corpus = M.MMIMDbCorpus(*M.synthetic_features(SAMPLES), dev)
    out = {"timing": "evaluation = one epoch's validation between a pair of device events and a host clock (it ends in "
                     "its read-back); replay = one pair of device events per graph replay (fused) or per eager B-row eval "
                     "forward + loss (per_pattern); zero_refresh = one pair per eager refresh; a round = the median of "
                     "its samples, a leg = the median of its round medians; rounds interleave the legs",
           "command": "python scripts/bench_mmimdb_patterns.py --out profiles/mmimdb_patterns.json",
           "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "model": "MMIMDb GMU: 4096 / 300 -> 512, hidden 512, 23 genres", "patterns": list(PATTERNS),
           "samples": SAMPLES, "runs": a.runs, "evaluations_per_round": a.evaluations, "replays_per_round": a.replays,
           "default_fusion": M.DEFAULT_PATTERN_FUSION, "by_batch": {}}
    for B in BATCHES:
        out["by_batch"][str(B)] = bench_batch(model, corpus, B, a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
