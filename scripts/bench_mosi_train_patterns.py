#!/usr/bin/env python
"""What training every missing-modality pattern of a batch in one step costs: three captured train steps on the same model
and optimizer, timed one after the other in one process —

  (a) ``plain``       ``FusedMosiStep`` at B rows: today's step, one pattern per sample;
  (b) ``patterns``    ``FusedMosiPatternStep`` at B rows: every row under all seven patterns (encoders forward and backward
                      over 2B rows, the classifier over 7B rows, ``tspm_pattern_expand`` and its adjoint);
  (c) ``replicated``  ``FusedMosiStep`` on the replicated 7B-row batch: how a user gets (b)'s gradient without it.  Where
                      the plain step refuses that row count the refusal is recorded instead of a time.

Shapes (Ta, Tv, Tt): MOSI aligned 50 at B = 128, MOSI (375, 500, 50) at B = 128, MOSEI (500, 375, 50) at B = 256.

Protocol: every step is built on random inputs and called three times (eager, capture, replay); then ``--runs`` rounds (5),
each timing the legs one after the other (interleaved), ``--replays`` replays of the leg's captured graph per round, each
between its own pair of device events; a round's figure is the median of its replays, a leg's the median of its round
medians, with their range.  ``expand_bwd``: ``tspm_pattern_expand_bwd`` alone at the shape's (B, 7, widths), one pair of
device events per launch (a launch-bound figure: the kernel moves 9B x E floats).  The replays keep training on the same
batch (Adam steps included); the masks are the device's own draws.

Nothing in the package depends on the result.  Needs the MI355X: there is no CPU leg.

    python scripts/bench_mosi_train_patterns.py --out profiles/mosi_train_patterns.json
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SHAPES = {"mosi_aligned": ("mosi", 128, 50), "mosi": ("mosi", 128, (375, 500, 50)), "mosei": ("mosei", 256, (500, 375, 50))}
LEGS = ("plain", "patterns", "replicated")


def replay_median(graph, n):
    import torch
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for e0, e1 in ev:
        e0.record()
        graph.replay()
        e1.record()
    torch.cuda.synchronize()
    return statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)


def expand_bwd_median(batch, widths, n, dev):
    import torch
    from tspm_amd import _lib as L
    from tspm_amd import mosi as M
    P, E = len(M.ALL_PATTERNS), sum(widths)
    keep = (ctypes.c_int32 * (3 * P))(*[int(ch in p) for p in M.ALL_PATTERNS for ch in "avt"])
    dout, demb = torch.randn(P * batch, E, device=dev), torch.empty(2 * batch, E, device=dev)
    sh = L.stream_handle()

    def launch():
        L.check(L.lib().tspm_pattern_expand_bwd(batch, P, keep, *widths, dout.data_ptr(), E, demb.data_ptr(), E, 7, sh),
                "pattern_expand_bwd")
    for _ in range(10):
        launch()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for e0, e1 in ev:
        e0.record()
        launch()
        e1.record()
    torch.cuda.synchronize()
    t = [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]
    return {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t), "launches": n,
            "bytes_moved": 4 * E * (P + 2) * batch}


def time_shape(key, a):
    import torch
    import tspm_amd
    from tspm_amd import mosi as M
    name, batch, steps = SHAPES[key]
    dev = torch.device("cuda", 0)
    c = M.YAML_CONFIGS[name]
    P = len(M.ALL_PATTERNS)
    torch.manual_seed(3)
    model = M.build_utt_fusion(name).to(dev)
    opt = tspm_amd.FusedAdam(model.parameters(), lr=c["lr"], weight_decay=c["weight_decay"])
    g = torch.Generator().manual_seed(1234)
    feats = (c["audio_dim"], c["video_dim"], c["text_dim"])

    def batch_of(n):
        x = [s * torch.randn(n, t, f, generator=g) for s, t, f in zip((1.0, 0.5, 0.3), M.steps_triple(steps), feats)]
        return [t.to(dev) for t in x] + [torch.randint(0, 3, (n,), generator=g).to(dev)]
    build = {"plain": lambda: (model.fused_step(opt, None, batch, steps), batch),
             "patterns": lambda: (model.fused_pattern_step(opt, None, batch, steps), batch),
             "replicated": lambda: (model.fused_step(opt, None, P * batch, steps), P * batch)}
    graphs, refused, losses = {}, {}, {}
    for leg in LEGS:
        try:
            st, n = build[leg]()
            data = batch_of(n)
            for _ in range(3):  # eager, capture, replay
                out = st.step(*data)
            torch.cuda.synchronize()
        except tspm_amd.TspmError as e:
            if leg != "replicated":
                raise
            refused[leg] = str(e)
            continue
        losses[leg] = float(out["loss"].item())
        if st.graph is None or not (losses[leg] == losses[leg]):
            raise SystemExit(f"{key} {leg}: no captured graph or a NaN loss ({losses[leg]})")
        graphs[leg] = st.graph
    replays = a.replays if isinstance(steps, int) else a.long_replays
    rounds = {leg: [] for leg in graphs}
    for _ in range(a.runs):  # interleaved
        for leg in graphs:
            rounds[leg].append(replay_median(graphs[leg], replays))
    widths = (model.netA.hidden_size, model.netV.hidden_size, model.netT.hidden_size)
    out = {"model": name, "batch": batch, "steps": list(M.steps_triple(steps)), "patterns": P,
           "rows": {"plain": batch, "patterns": {"encoders": 2 * batch, "classifier": P * batch}, "replicated": P * batch},
           "replays_per_round": replays, "legs": {}, "refused": refused,
           "expand_bwd": expand_bwd_median(batch, widths, a.replays, dev)}
    for leg, r in rounds.items():
        out["legs"][leg] = {"replay_median_us": statistics.median(r), "replay_min_us": min(r), "replay_max_us": max(r),
                            "round_medians_us": r, "loss_after_warmup": losses[leg]}
    med = {leg: v["replay_median_us"] for leg, v in out["legs"].items()}
    out["ratios"] = {"patterns_over_plain": med["patterns"] / med["plain"]}
    if "replicated" in med:
        out["ratios"]["patterns_over_replicated"] = med["patterns"] / med["replicated"]
        out["ratios"]["replicated_over_plain"] = med["replicated"] / med["plain"]
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--replays", type=int, default=200, help="timed graph replays per leg and round at the aligned shape")
    ap.add_argument("--long-replays", type=int, default=30, help="... at the unaligned shapes")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mosi_train_patterns.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mosi_train_patterns: needs the MI355X (no CPU leg)")
    result = {"timing": "one pair of device events per replay of a leg's captured train-step graph; a round = the median "
                        "of its replays, a leg = the median of its round medians; rounds interleave the legs; expand_bwd = "
                        "one pair of device events per launch of tspm_pattern_expand_bwd alone",
              "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
              "runs": a.runs, "shapes": {}}
    for key in [k for k in a.shapes.split(",") if k]:
        result["shapes"][key] = r = time_shape(key, a)
        print(key, {leg: round(v["replay_median_us"], 1) for leg, v in r["legs"].items()}, r["ratios"],
              {"expand_bwd_us": round(r["expand_bwd"]["median_us"], 2)}, r["refused"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
