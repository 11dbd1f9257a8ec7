#!/usr/bin/env python
"""Frozen encoders and per-group Adam in the UTT-Fusion fused step: what the step costs with two FusedAdam groups and
with one, two or all three encoders frozen, next to the one-group, all-trainable step at the same shape.

Shapes: MOSI aligned 50 at B = 128; unaligned MOSI (375, 500, 50) at B = 128; unaligned MOSEI (500, 375, 50) at B = 256.

Legs, each the graph-replayed fused train step (``mosi.finetune_param_groups`` builds the groups):

* ``f1``: one group, every parameter trainable (the step as it always was);
* ``f2``: two groups (classifier at the YAML's lr / wd, encoders at lr / 10, wd 0), every parameter trainable;
* ``za``: audio + video frozen;  ``zt``: text frozen;  ``z3``: all three frozen (one group: the classifier).

Protocol: every leg is timed ``--runs`` times (5), the legs interleaved within each run; a run is
``--steps`` replays (``--long-steps`` at the unaligned shapes), each between its own pair of device events; a run's figure
is the median of its samples, a leg's the median [min, max] of its runs.  Recorded per leg as well: the optimizer phase's
launch record of an eager step (the tspm_* calls whose name holds "adam" or "clip_coef"; the clip call is two launches),
and the frozen set.  ``--ab-from FILE`` copies the ``ab_aligned`` block of a ``bench_mosi_unaligned.py --ab-lib`` result
into the profile.

Nothing in the package depends on the result.  Needs the MI355X: there is no CPU leg.

    python scripts/bench_mosi_finetune.py --out profiles/mosi_finetune.json [--ab-from other.json]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SHAPES = {"mosi_aligned": ("mosi", 128, 50), "mosi": ("mosi", 128, (375, 500, 50)),
          "mosei": ("mosei", 256, (500, 375, 50))}
LEGS = {"f1": dict(two=False, freeze=()), "f2": dict(two=True, freeze=()),
        "za": dict(two=True, freeze=("audio", "video")), "zt": dict(two=True, freeze=("text",)),
        "z3": dict(two=True, freeze=("audio", "video", "text"))}
LAUNCHES = {"tspm_grad_clip_coef": 2, "tspm_grad_clip_coef_multi": 2}  # every other optimizer call is one launch


def timed(fn, n):
    import torch
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]


class Recorder:
    """``_lib.lib()`` with every tspm_* call noted by name."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("tspm_"):
            return fn

        def call(*args):
            self.calls.append(name)
            return fn(*args)
        return call


def build(name, batch, steps, leg, seed=3):
    import torch
    import tspm_amd
    from tspm_amd import mosi as M
    dev = torch.device("cuda", 0)
    c = M.YAML_CONFIGS[name]
    torch.manual_seed(seed)
    model = M.build_utt_fusion(name).to(dev)
    kw = dict(encoder_lr=c["lr"] / 10, encoder_weight_decay=0.0) if LEGS[leg]["two"] else {}
    groups = M.finetune_param_groups(model, lr=c["lr"], weight_decay=c["weight_decay"], freeze=LEGS[leg]["freeze"], **kw)
    opt = tspm_amd.FusedAdam(groups)
    st = M.FusedMosiStep(model, opt, None, batch, steps)
    ta, tv, tt = M.steps_triple(steps)
    g = torch.Generator().manual_seed(1234)
    A = torch.randn(batch, ta, c["audio_dim"], generator=g).to(dev)
    V = (0.5 * torch.randn(batch, tv, c["video_dim"], generator=g)).to(dev)
    T = (0.3 * torch.randn(batch, tt, c["text_dim"], generator=g)).to(dev)
    y = torch.randint(0, 3, (batch,), generator=g).to(dev)
    st.eng.load(A, V, T, y)
    return model, opt, st


def over_runs(medians):
    return {"run_medians_us": medians, "min_us": min(medians), "max_us": max(medians),
            "median_us": statistics.median(medians)}


def time_shape(key, a):
    import torch
    from tspm_amd import _lib as L
    from tspm_amd import mosi as M
    name, batch, steps = SHAPES[key]
    n = a.steps if isinstance(steps, int) else a.long_steps
    built, records = {}, {}
    real = L.lib
    for leg in LEGS:
        model, opt, st = built[leg] = build(name, batch, steps, leg)
        rec = Recorder(real())
        L.lib = lambda rec=rec: rec  # the first (eager) step's launch record
        try:
            st.run()
        finally:
            L.lib = real
        records[leg] = rec.calls
        for _ in range(a.warmup):  # capture, replays
            st.run()
        torch.cuda.synchronize()
        if st.graph is None or not math.isfinite(st.eng.loss.item()):
            raise SystemExit(f"{key} {leg}: the step was not captured or its loss is not finite")
    samples = {leg: [] for leg in LEGS}
    for _ in range(a.runs):
        for leg in LEGS:
            st = built[leg][2]
            st.run()
            torch.cuda.synchronize()
            samples[leg].append(statistics.median(timed(st.graph.replay, n)))
    out = {"model": name, "batch": batch, "steps": list(M.steps_triple(steps)), "samples_per_run": n, "legs": {}}
    for leg in LEGS:
        model, opt, st = built[leg]
        if not math.isfinite(st.eng.loss.item()):
            raise SystemExit(f"{key} {leg}: non-finite loss")
        calls = records[leg]
        optc = [c for c in calls if "adam" in c or "clip_coef" in c]
        out["legs"][leg] = dict(
            step=over_runs(samples[leg]), frozen=list(st.frozen), groups=len(opt.flat_groups()),
            optimizer_calls=optc, optimizer_launches=sum(LAUNCHES.get(c, 1) for c in optc),
            lstm_bwd_calls=sum(c.startswith("tspm_lstm_bwd") for c in calls),
            lstm_wgrad_calls=calls.count("tspm_linear_bwd_weight_splitk"),
            textcnn_bwd_calls=calls.count("tspm_textcnn_bwd"), calls_per_step=len(calls))
    base = out["legs"]["f1"]["step"]
    out["ratios_to_f1"] = {leg: out["legs"][leg]["step"]["median_us"] / base["median_us"] for leg in LEGS if leg != "f1"}
    out["f2_within_f1_range"] = bool(base["min_us"] <= out["legs"]["f2"]["step"]["median_us"] <= base["max_us"])
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=300, help="timed replays per run at the aligned shape")
    ap.add_argument("--long-steps", type=int, default=40, help="timed replays per run at the unaligned shapes")
    ap.add_argument("--runs", type=int, default=5, help="runs per leg (legs interleaved within a run)")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--shapes", default=",".join(SHAPES), help="comma-separated subset of: " + ", ".join(SHAPES))
    ap.add_argument("--ab-from", default=None, help="a bench_mosi_unaligned.py --ab-lib result whose ab_aligned to record")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mosi_finetune.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mosi_finetune: needs the MI355X (no CPU leg)")
    result = {"timing": "one pair of device events per graph replay; a run = the median of its samples; per leg the "
                        "median [min, max] over the runs; legs interleaved within each run",
              "legs": {k: dict(groups=2 if v["two"] and len(v["freeze"]) < 3 else 1, freeze=list(v["freeze"]))
                       for k, v in LEGS.items()},
              "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
              "shapes": {}}
    if a.ab_from:
        with open(a.ab_from) as f:
            result["ab_aligned"] = json.load(f)["ab_aligned"]
    for key in [k for k in a.shapes.split(",") if k]:
        result["shapes"][key] = r = time_shape(key, a)
        for leg, v in r["legs"].items():
            s = v["step"]
            print(f"{key} {leg}: step {s['median_us']:.1f} us [{s['min_us']:.1f}, {s['max_us']:.1f}]  optimizer launches "
                  f"{v['optimizer_launches']}  lstm_bwd {v['lstm_bwd_calls']} textcnn_bwd {v['textcnn_bwd_calls']}",
                  flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out, "ab_aligned": {k: v for k, v in result.get("ab_aligned", {}).items() if k != "runs"}}))


if __name__ == "__main__":
    main()
