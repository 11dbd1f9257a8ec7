#!/usr/bin/env python
"""What training every missing-modality pattern of an MMIMDb batch in one step costs and saves: the all-pattern step
(``FusedMMIMDbPatternStep``: encoders over B + 1 rows, fusion and classifier over 3·B) next to the two ways of getting
the same update today — the plain ``FusedMMIMDbStep`` on the explicitly replicated and masked 3·B-row batch — and next to
the plain B-row step, which trains one pattern.

The GMU model of BASELINE configs[3] (4096 / 300 -> 512, hidden 512, 23 genres) on ``mmimdb.synthetic_features``, all
three patterns, B = 128 and 256.  Legs, all in one process, each with its own model and FusedAdam from the same seed:

    plain_B          FusedMMIMDbStep at B                       (one pattern; the floor)
    pattern_kernel   FusedMMIMDbPatternStep at B, fusion="kernel"    (tspm_gmu_pattern_fwd / tspm_gmu_pattern_bwd)
    pattern_launches FusedMMIMDbPatternStep at B, fusion="launches"  (expand + the engine's fusion + expand_bwd + sum)
    plain_3B         FusedMMIMDbStep at 3·B on the replicated batch  (the same mathematical step)
    gmu_pattern_bwd  tspm_gmu_pattern_bwd alone (its two launches), on the pattern_kernel step's buffers
    bn1d_fwd_rep_pair tspm_bn1d_fwd_rep_pair alone, on the pattern_kernel step's buffers (running statistics NULL)

Protocol: every step leg is warmed up (``--warmup`` steps: eager, capture, replay); then ``--runs`` rounds, each timing
the legs one after the other (interleaved): ``--replays`` graph replays (or eager calls of an entry point) per leg and
round, one pair of device events each.  A round's figure is the median of its samples, a leg's the median of its round
medians, with their range.  A replay is the whole step: forward, loss, backward, Adam.  The first step of the
pattern_kernel and plain_3B legs, from the same weights and dropout masks, are compared inside (loss within 1e-4
relative), else the script fails.  Nothing in the package reads the result; ``mmimdb.DEFAULT_TRAIN_PATTERN_FUSION``
records which leg measured faster at B = 256.  Needs the MI355X: there is no CPU leg.

    python scripts/bench_mmimdb_train_patterns.py --out profiles/mmimdb_train_patterns.json
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

BATCHES, PATTERNS = (128, 256), ("it", "i", "t")
STEP_LEGS = ("plain_B", "pattern_kernel", "pattern_launches", "plain_3B")
OP_LEGS = ("gmu_pattern_bwd", "bn1d_fwd_rep_pair")
LR, WD = 1e-5, 1e-3


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


def build(dev):
    import torch
    import tspm_amd
    from tspm_amd import mmimdb as M
    torch.manual_seed(0)
    model = M.MMIMDb(M.MMIMDbModalityEncoder(4096, 512), M.MMIMDbModalityEncoder(300, 512),
                     gated_bimodal_network=M.GatedBiModalNetwork(input_one_dim=512, output_one_dim=512,
                                                                 input_two_dim=512, output_two_dim=512),
                     classifier=M.MLPGenreClassifier(input_size=512, hidden_size=512, output_size=23)).to(dev)
    return model, tspm_amd.FusedAdam(model.parameters(), lr=LR, weight_decay=WD)


def bench_batch(dev, B, a):
    import torch
    from tspm_amd import _lib as L
    from tspm_amd import mmimdb as M
    P = len(PATTERNS)
    I, T, y = (t.to(dev) for t in M.synthetic_features(B, seed=1234 + B))
    Ir = torch.cat([I * M.PATTERNS[p][0] for p in PATTERNS])
    Tr = torch.cat([T * M.PATTERNS[p][1] for p in PATTERNS])
    yr = y.repeat(P, 1)
    keep = (torch.rand(2, P * B, 512, generator=torch.Generator().manual_seed(B)) >= 0.5).to(torch.uint8).to(dev)
    steps, first = {}, {}
    for leg in STEP_LEGS:
        model, opt = build(dev)
        if leg == "plain_B":
            st, args = M.FusedMMIMDbStep(model, opt, None, B), (I, T, y)
        elif leg == "plain_3B":
            st, args = M.FusedMMIMDbStep(model, opt, None, P * B), (Ir, Tr, yr)
        else:
            st = M.FusedMMIMDbPatternStep(model, opt, None, B, patterns=PATTERNS, fusion=leg.split("_")[1])
            args = (I, T, y)
            if st.fusion != leg.split("_")[1]:
                raise SystemExit(f"{leg}: built the {st.fusion} leg")
        if leg != "plain_B":
            st.keep_override = keep
        first[leg] = float(st.step(*args)["loss"].item())
        st.keep_override = None
        for _ in range(a.warmup - 1):
            st.step(*args)
        torch.cuda.synchronize()
        if st.graph is None:
            raise SystemExit(f"{leg}: no graph after {a.warmup} steps")
        steps[leg] = st
    ref = first["plain_3B"]
    agree = {leg: abs(first[leg] - ref) / abs(ref) for leg in ("pattern_kernel", "pattern_launches")}
    if max(agree.values()) > 1e-4:
        raise SystemExit(f"B={B}: first-step loss differs from the replicated plain step's: {first}")
    # the two entry points alone, on the kernel leg's buffers (contents of a finished step)
    st = steps["pattern_kernel"]
    enc, clf, d, sh, lib = st.enc, st.clf, st.enc.d, L.stream_handle(), L.lib()
    wz = st.model.fusion_module.hidden_sigmoid.weight
    scratch_du, scratch_ds = torch.empty_like(enc.dU), torch.empty_like(clf.ds)

    def gmu_bwd():
        L.check(lib.tspm_gmu_pattern_bwd(B, P, st._keep, d, clf.dZ.data_ptr(), d, clf.H.data_ptr(), 2 * d,
                                         clf.gate.data_ptr(), wz.data_ptr(), scratch_du.data_ptr(), 2 * d,
                                         scratch_ds.data_ptr(), st.ws.data_ptr(), st.ws.numel() * 4, sh),
                "gmu_pattern_bwd")
    bn_args, bn_bufs = [], []  # all three patterns: each modality kept by two, dropped by one
    for bn, x, width in ((st.model.text_model.net[0], enc.T, enc.dt), (st.model.image_model.net[0], enc.I, enc.di)):
        mean, inv = torch.empty(width, device=dev), torch.empty(width, device=dev)
        y_out = torch.empty(B + 1, width, device=dev)
        bn_bufs += [mean, inv, y_out]
        bn_args += [width, x.data_ptr(), bn.weight.data_ptr(), bn.bias.data_ptr(), None, None, 0.1, float(bn.eps),
                    mean.data_ptr(), inv.data_ptr(), y_out.data_ptr(), 2, 1]

    def bn_rep():
        L.check(lib.tspm_bn1d_fwd_rep_pair(B, *bn_args, sh), "bn1d_fwd_rep_pair")
    ops = {"gmu_pattern_bwd": gmu_bwd, "bn1d_fwd_rep_pair": bn_rep}
    for fn in ops.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    rounds = {leg: [] for leg in STEP_LEGS + OP_LEGS}
    for _ in range(a.runs):  # interleaved
        for leg in STEP_LEGS:
            rounds[leg].append(timed_calls(steps[leg].graph.replay, a.replays))
        for leg in OP_LEGS:
            rounds[leg].append(timed_calls(ops[leg], a.replays))
    del bn_bufs
    out = {"batch": B, "rows": {"plain_B": B, "pattern_encoders": B + 1, "pattern_fusion_classifier": P * B,
                                "plain_3B": P * B},
           "legs": {leg: spread(v) for leg, v in rounds.items()},
           "first_step_loss": first, "first_step_loss_rel_diff_vs_plain_3B": agree}
    med = lambda leg: out["legs"][leg]["median_us"]  # noqa: E731
    out["ratios"] = {"pattern_kernel_over_plain_3B": med("pattern_kernel") / med("plain_3B"),
                     "pattern_launches_over_plain_3B": med("pattern_launches") / med("plain_3B"),
                     "pattern_kernel_over_plain_B": med("pattern_kernel") / med("plain_B"),
                     "pattern_launches_over_plain_B": med("pattern_launches") / med("plain_B"),
                     "plain_3B_over_plain_B": med("plain_3B") / med("plain_B"),
                     "pattern_kernel_over_three_plain_B": med("pattern_kernel") / (3 * med("plain_B"))}
    out["fusion"] = {"kernel_us": med("pattern_kernel"), "launches_us": med("pattern_launches"),
                     "faster": "kernel" if med("pattern_kernel") <= med("pattern_launches") else "launches"}
    print(B, {leg: round(med(leg), 1) for leg in rounds}, out["ratios"], out["fusion"], flush=True)
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--warmup", type=int, default=5, help="untimed steps per leg (eager, capture, replays)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--replays", type=int, default=200, help="timed graph replays / entry-point calls per leg and round")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mmimdb_train_patterns.json"))
    a = ap.parse_args()
    if a.warmup < 2:
        raise SystemExit("bench_mmimdb_train_patterns: --warmup >= 2 (the second call of a step captures its graph)")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mmimdb_train_patterns: needs the MI355X (no CPU leg)")
    import tspm_amd  # noqa: F401
    from tspm_amd import mmimdb as M
    dev = torch.device("cuda", 0)
    out = {"timing": "one pair of device events per graph replay of a whole step (forward, loss, backward, Adam) or per "
                     "eager call of an entry point; a round = the median of its samples, a leg = the median of its "
                     "round medians; rounds interleave the legs",
           "command": "python scripts/bench_mmimdb_train_patterns.py --out profiles/mmimdb_train_patterns.json",
           "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "model": "MMIMDb GMU: 4096 / 300 -> 512, hidden 512, 23 genres", "patterns": list(PATTERNS),
           "runs": a.runs, "replays_per_round": a.replays, "default_fusion": M.DEFAULT_TRAIN_PATTERN_FUSION,
           "by_batch": {}}
    for B in BATCHES:
        out["by_batch"][str(B)] = bench_batch(dev, B, a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
