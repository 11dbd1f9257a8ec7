#!/usr/bin/env python
"""Per-sample sequence lengths on the unaligned MOSI / MOSEI shapes: what the ragged mode of the UTT-Fusion step
(tspm_lstm_fwd_len / tspm_lstm_bwd_len) costs and saves against the unmasked step at the same padded length.

Shapes (Ta, Tv, Tt): ``mosi`` (375, 500, 50) at B = 128 ("last"), ``mosei`` (500, 375, 50) at B = 256 ("maxpool", 16-bit
index).  Legs, each the graph-replayed fused train step and the step's two recurrence launches alone:

* ``a``: the existing unmasked path (``FusedMosiStep(ragged=False)``);
* ``b``: ragged mode, every length equal to the padded length — the cost of the feature itself;
* ``c``: ragged mode, seeded lengths uniform in [T/10, T/2] per modality — the batch's longest sequence is about half
  the padding;
* ``d``: ragged mode, seeded lengths uniform in [T/10, T] — some row is near the full length.

The length distributions of (c) and (d) are SYNTHETIC: the real corpora are not part of this repository.  (b), (c), (d)
run on ONE ragged step and one captured graph; only the contents of its length buffers change between legs.

Every leg is timed ``--runs`` times (5), the legs interleaved within each run; a run is ``--steps`` replays / launches,
each between its own pair of device events (the timing of scripts/bench_mosi_unaligned.py), summarised by its median.
Reported per leg: the runs' medians, their min–max range and median; then (b)/(a), (c)/(a) and (d)/(a) on the medians
of medians, (c) next to the ratio of the batch's longest sequence to the padded length, and whether (b) lies inside
(a)'s own min–max range.  No threshold is applied: the numbers are the result.

    python scripts/bench_mosi_lengths.py --out profiles/mosi_lengths.json

``--text`` times the text modality's lengths instead (``text_lengths``: tspm_textcnn_pool_fwd_len), on the same shapes,
with the same interleaving and summary, into ``--text-out``.  Legs, each the graph-replayed fused train step and the
step's pooling launch alone:

* ``ra``: the ragged step without ``text_lengths``, every length at the padded length;
* ``tb``: the ragged step with ``text_lengths``, every length at the padded length — the cost of the feature itself;
* ``rc``: the ragged step without ``text_lengths``, leg (c)'s seeded audio / video lengths;
* ``tc``: the ragged step with ``text_lengths``, the same audio / video lengths and seeded text lengths uniform in
  [0.4 T, T] (20..50 of 50 steps, the range of ``bench.py --mosi``'s synthetic corpus) — SYNTHETIC as well.

Reported: (tb)/(ra) and (tc)/(rc) on the medians of medians, and whether (tb) lies inside (ra)'s and (tc) inside (rc)'s own
min–max range.

    python scripts/bench_mosi_lengths.py --text --text-out profiles/mosi_text_lengths.json
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (REPO, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_mosi_unaligned import SHAPES, summarise, timed  # noqa: E402

LEGS = ("a", "b", "c", "d")
LEG_RANGE = {"b": (1.0, 1.0), "c": (0.1, 0.5), "d": (0.1, 1.0)}  # lengths uniform in [lo * T, hi * T]


def build(name, batch, steps, ragged, seed=3, text_lengths=False):
    import torch
    import tspm_amd
    from tspm_amd import mosi as M
    dev = torch.device("cuda", 0)
    c = M.YAML_CONFIGS[name]
    torch.manual_seed(seed)
    model = M.build_utt_fusion(name).to(dev)
    opt = tspm_amd.FusedAdam(model.parameters(), lr=c["lr"], weight_decay=c["weight_decay"])
    st = M.FusedMosiStep(model, opt, None, batch, steps, ragged=ragged, text_lengths=text_lengths)
    ta, tv, tt = M.steps_triple(steps)
    g = torch.Generator().manual_seed(1234)
    A = torch.randn(batch, ta, c["audio_dim"], generator=g).to(dev)
    V = (0.5 * torch.randn(batch, tv, c["video_dim"], generator=g)).to(dev)
    T = (0.3 * torch.randn(batch, tt, c["text_dim"], generator=g)).to(dev)
    y = torch.randint(0, 3, (batch,), generator=g).to(dev)
    st.eng.load(A, V, T, y)
    return model, st


def leg_lengths(leg, batch, steps, seed=7):
    """{"audio": int32 [B], "video": int32 [B]} of a ragged leg (host tensors), seeded per leg and modality."""
    import torch
    lo, hi = LEG_RANGE[leg]
    out = {}
    for i, (nm, t) in enumerate(zip(("audio", "video"), steps[:2])):
        g = torch.Generator().manual_seed(seed * 100 + ord(leg) * 2 + i)
        a, b = max(1, int(round(lo * t))), int(round(hi * t))
        out[nm] = torch.randint(a, b + 1, (batch,), generator=g, dtype=torch.int32)
    return out


def recurrence_calls(model, st):
    """The step's two recurrence launches alone, as the step issues them, on the buffers the step filled."""
    from tspm_amd import _lib as L
    from tspm_amd import mosi as M
    e, sh = st.eng, L.stream_handle()
    ta, tv, _ = e.Ts
    fd = ((L.LstmFwdLenDesc if e.ragged else L.LstmFwdDesc) * 2)()
    bd = ((L.LstmBwdLenDesc if e.ragged else L.LstmBwdDesc) * 2)()
    for i, (nm, enc, x, col, t) in enumerate((("a", model.netA, e.A, 0, ta),
                                              ("v", model.netV, e.V, model.netA.hidden_size, tv))):
        M._lstm_fwd_prepare(fd[i], enc, x, e.lstm[nm], e.B, t, e.fused.data_ptr() + col * 4, e.E, sh)
        M._lstm_bwd_desc(bd[i], enc, e.lstm[nm], e.B, t, e.dfused.data_ptr() + col * 4, e.E)
        if e.ragged:
            M._len_desc(fd[i], e.lens[nm], e.wide)
            M._len_desc(bd[i], e.lens[nm], e.wide)
    if e.ragged:
        return (lambda: L.check(L.lstm_fwd_len(2, fd, sh), "lstm_fwd_len"),
                lambda: L.check(L.lstm_bwd_len(2, bd, sh), "lstm_bwd_len"))
    return (lambda: L.check(L.lstm_fwd(2, fd, sh, e.wide), "lstm_fwd"),
            lambda: L.check(L.lstm_bwd(2, bd, sh, e.wide), "lstm_bwd"))


TEXT_LEGS = ("ra", "tb", "rc", "tc")
TEXT_RANGE = (0.4, 1.0)  # text lengths of leg tc uniform in [lo * Tt, hi * Tt]


def text_leg_lengths(leg, batch, steps, seed=7):
    """The length dict of a ``--text`` leg: None (every buffer at the padded length) for ra / tb, leg (c)'s audio / video
    lengths for rc / tc, plus seeded text lengths for tc."""
    import torch
    if leg in ("ra", "tb"):
        return None
    out = leg_lengths("c", batch, steps, seed)
    if leg == "tc":
        g = torch.Generator().manual_seed(seed * 100 + 99)
        lo, hi = TEXT_RANGE
        out["text"] = torch.randint(max(1, int(round(lo * steps[2]))), int(round(hi * steps[2])) + 1, (batch,),
                                    generator=g, dtype=torch.int32)
    return out


def pool_call(model, st):
    """The step's TextCNN pooling launch alone, as mosi._text_forward issues it, on the buffers the step filled."""
    import ctypes
    from tspm_amd import _lib as L
    e, t, sh, lib = st.eng, model.netT, L.stream_handle(), L.lib()
    heights = (ctypes.c_int32 * 3)(*t.heights)
    outs = (ctypes.c_void_p * 3)(*[y.data_ptr() for y in e.conv_out])
    biases = (ctypes.c_void_p * 3)(*[cv.bias.data_ptr() for cv in t.convs()])
    tp = t.dropout.p
    args = (e.B, e.Tt, 3, heights, e.C, outs, biases, e.keeps[0].data_ptr(), 1.0 / (1.0 - tp) if tp < 1 else 0.0,
            e.pooled.data_ptr(), e.argmax.data_ptr(), e.fc_in.data_ptr(), e.nc)
    if e.text_lens is not None:
        return lambda: L.check(lib.tspm_textcnn_pool_fwd_len(*args, e.text_lens.data_ptr(), sh), "textcnn_pool_fwd_len")
    return lambda: L.check(lib.tspm_textcnn_pool_fwd(*args, sh), "textcnn_pool_fwd")


def time_text_shape(key, a):
    import torch
    from tspm_amd import mosi as M
    name, batch, steps = SHAPES[key]
    steps3 = M.steps_triple(steps)
    built = {tl: build(name, batch, steps, True, text_lengths=tl) for tl in (False, True)}
    for model, st in built.values():
        for _ in range(a.warmup):  # eager, capture, replays
            st.run()
        torch.cuda.synchronize()
        if st.graph is None or not math.isfinite(st.eng.loss.item()):
            raise SystemExit(f"{key}: the step was not captured or its loss is not finite")
    pools = {tl: pool_call(*built[tl]) for tl in built}
    lengths = {leg: text_leg_lengths(leg, batch, steps3) for leg in TEXT_LEGS}
    graphs = {tl: built[tl][1].graph for tl in built}
    samples = {leg: {"step": [], "pool": []} for leg in TEXT_LEGS}
    for _ in range(a.runs):
        for leg in TEXT_LEGS:
            tl = leg[0] == "t"
            model, st = built[tl]
            ln = lengths[leg]
            st.eng.set_lengths(None if ln is None else {k: v.to(st.eng.device) for k, v in ln.items()})
            st.run()
            torch.cuda.synchronize()
            samples[leg]["step"].append(statistics.median(timed(st.graph.replay, a.steps)))
            samples[leg]["pool"].append(statistics.median(timed(pools[tl], a.steps)))
    if any(built[tl][1].graph is not graphs[tl] for tl in built):
        raise SystemExit(f"{key}: a step was recaptured between legs")
    if not all(math.isfinite(st.eng.loss.item()) for _, st in built.values()):
        raise SystemExit(f"{key}: non-finite loss")
    out = {"model": name, "batch": batch, "steps": list(steps3), "legs": {}}
    for leg in TEXT_LEGS:
        out["legs"][leg] = r = {k: over_runs(v) for k, v in samples[leg].items()}
        if lengths[leg] is not None:
            r["lengths"] = {nm: {"min": int(v.min()), "max": int(v.max()), "mean": float(v.float().mean())}
                            for nm, v in lengths[leg].items()}
            r["synthetic_lengths"] = True
    out["ratios"], out["within_base_range"] = {}, {}
    for leg, base in (("tb", "ra"), ("tc", "rc")):
        r, b = out["legs"][leg], out["legs"][base]
        out["ratios"][f"{leg}/{base}"] = {k: r[k]["median_us"] / b[k]["median_us"] for k in ("step", "pool")}
        out["within_base_range"][f"{leg} in {base}"] = {
            k: bool(b[k]["min_us"] <= r[k]["median_us"] <= b[k]["max_us"]) for k in ("step", "pool")}
    return out


def over_runs(medians):
    return {"run_medians_us": medians, "min_us": min(medians), "max_us": max(medians),
            "median_us": statistics.median(medians)}


def time_shape(key, a):
    import torch
    from tspm_amd import mosi as M
    name, batch, steps = SHAPES[key]
    steps3 = M.steps_triple(steps)
    built = {False: build(name, batch, steps, False), True: build(name, batch, steps, True)}
    for model, st in built.values():
        for _ in range(a.warmup):  # eager, capture, replays
            st.run()
        torch.cuda.synchronize()
        if st.graph is None or not math.isfinite(st.eng.loss.item()):
            raise SystemExit(f"{key}: the step was not captured or its loss is not finite")
    calls = {r: recurrence_calls(*built[r]) for r in built}
    lengths = {leg: leg_lengths(leg, batch, steps3) for leg in LEGS if leg != "a"}
    graph = built[True][1].graph
    samples = {leg: {"step": [], "fwd": [], "bwd": []} for leg in LEGS}
    for _ in range(a.runs):
        for leg in LEGS:
            model, st = built[leg != "a"]
            if leg != "a":
                st.eng.set_lengths({k: v.to(st.eng.device) for k, v in lengths[leg].items()})
            fwd, bwd = calls[leg != "a"]
            st.run()  # the saved activations of this leg's lengths, for the recurrences timed alone below
            torch.cuda.synchronize()
            samples[leg]["step"].append(statistics.median(timed(st.graph.replay, a.steps)))
            samples[leg]["fwd"].append(statistics.median(timed(fwd, a.steps)))
            samples[leg]["bwd"].append(statistics.median(timed(bwd, a.steps)))
    if built[True][1].graph is not graph:
        raise SystemExit(f"{key}: the ragged step was recaptured between legs")
    if not all(math.isfinite(st.eng.loss.item()) for _, st in built.values()):
        raise SystemExit(f"{key}: non-finite loss")
    out = {"model": name, "batch": batch, "steps": list(steps3), "wide_index": bool(built[True][1].eng.wide),
           "legs": {}}
    for leg in LEGS:
        out["legs"][leg] = r = {k: over_runs(v) for k, v in samples[leg].items()}
        r["recurrences_us"] = r["fwd"]["median_us"] + r["bwd"]["median_us"]
        if leg != "a":
            r["lengths"] = {nm: {"min": int(v.min()), "max": int(v.max()), "mean": float(v.float().mean()),
                                 "longest_over_padded": float(v.max()) / t}
                            for (nm, v), t in zip(lengths[leg].items(), steps3[:2])}
            r["synthetic_lengths"] = leg in ("c", "d")
    base = out["legs"]["a"]
    out["ratios"] = {}
    for leg in ("b", "c", "d"):
        r = out["legs"][leg]
        out["ratios"][f"{leg}/a"] = {"step": r["step"]["median_us"] / base["step"]["median_us"],
                                     "fwd": r["fwd"]["median_us"] / base["fwd"]["median_us"],
                                     "bwd": r["bwd"]["median_us"] / base["bwd"]["median_us"],
                                     "recurrences": r["recurrences_us"] / base["recurrences_us"],
                                     "longest_over_padded": {nm: v["longest_over_padded"]
                                                             for nm, v in r["lengths"].items()}}
    out["b_within_a_range"] = {k: bool(base[k]["min_us"] <= out["legs"]["b"][k]["median_us"] <= base[k]["max_us"])
                               for k in ("step", "fwd", "bwd")}
    return out


def text_main(a) -> None:
    import torch
    result = {"timing": "one pair of device events per graph replay / per launch; a run's figure is the median of its "
                        "samples; legs interleaved within each run",
              "legs": {"ra": "ragged step without text_lengths, every length = the padded length",
                       "tb": "ragged step with text_lengths, every length = the padded length",
                       "rc": "ragged step without text_lengths, SYNTHETIC audio / video lengths of leg (c)",
                       "tc": "ragged step with text_lengths, the same audio / video lengths and SYNTHETIC text lengths "
                             "uniform in [0.4 Tt, Tt] (seeded)"},
              "note": "the real corpora's length distribution is not in this repository: the lengths are synthetic",
              "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
              "runs": a.runs, "samples_per_run": a.steps, "shapes": {}}
    for key in [k for k in a.shapes.split(",") if k]:
        result["shapes"][key] = r = time_text_shape(key, a)
        for leg in TEXT_LEGS:
            s = r["legs"][leg]
            print(f"{key} leg {leg}: step {s['step']['median_us']:.1f} us [{s['step']['min_us']:.1f}, "
                  f"{s['step']['max_us']:.1f}]  pool {s['pool']['median_us']:.1f} us [{s['pool']['min_us']:.1f}, "
                  f"{s['pool']['max_us']:.1f}]", flush=True)
        print(f"{key} ratios: " + json.dumps(r["ratios"]) + " within the base leg's range: " +
              json.dumps(r["within_base_range"]), flush=True)
    if a.merge:
        with open(a.merge) as f:
            other = json.load(f)
        if "ab_aligned" in other:
            result["ab_aligned"] = {k: v for k, v in other["ab_aligned"].items() if k != "runs"}
    os.makedirs(os.path.dirname(os.path.abspath(a.text_out)), exist_ok=True)
    with open(a.text_out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.text_out}))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=40, help="timed replays / launches per run")
    ap.add_argument("--runs", type=int, default=5, help="runs per leg (legs interleaved within a run)")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--shapes", default="mosi,mosei")
    ap.add_argument("--merge", default=None, help="a JSON file whose top-level keys are copied into the result (for "
                    "instance the ab_aligned block bench_mosi_unaligned.py --ab-lib wrote)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mosi_lengths.json"))
    ap.add_argument("--text", action="store_true", help="time the text_lengths legs (ra, tb, rc, tc) instead")
    ap.add_argument("--text-out", default=os.path.join(REPO, "profiles", "mosi_text_lengths.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mosi_lengths: needs the MI355X (no CPU leg)")
    if a.text:
        text_main(a)
        return
    result = {"timing": "one pair of device events per graph replay / per launch; a run's figure is the median of its "
                        "samples; legs interleaved within each run",
              "legs": {"a": "unmasked path", "b": "ragged, every length = the padded length",
                       "c": "ragged, SYNTHETIC lengths uniform in [T/10, T/2] per modality (seeded)",
                       "d": "ragged, SYNTHETIC lengths uniform in [T/10, T] per modality (seeded)"},
              "note": "the real corpora's length distribution is not in this repository: (c) and (d) are synthetic",
              "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
              "runs": a.runs, "samples_per_run": a.steps, "shapes": {}}
    for key in [k for k in a.shapes.split(",") if k]:
        result["shapes"][key] = r = time_shape(key, a)
        for leg in LEGS:
            s = r["legs"][leg]
            print(f"{key} leg {leg}: step {s['step']['median_us']:.1f} us [{s['step']['min_us']:.1f}, "
                  f"{s['step']['max_us']:.1f}]  fwd {s['fwd']['median_us']:.1f} us  bwd {s['bwd']['median_us']:.1f} us",
                  flush=True)
        print(f"{key} ratios: " + json.dumps(r["ratios"]) + " b within a's range: " + json.dumps(r["b_within_a_range"]),
              flush=True)
    if a.merge:
        with open(a.merge) as f:
            other = json.load(f)
        if "ab_aligned" in other:
            result["ab_aligned"] = {k: v for k, v in other["ab_aligned"].items() if k != "runs"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
