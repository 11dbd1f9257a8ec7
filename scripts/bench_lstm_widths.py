#!/usr/bin/env python
"""LSTM encoder widths on the UTT-Fusion HIP path: what the fused MOSI step and the recurrence kernels alone cost at
hidden widths 32, 64 and 128, and whether the 64-wide step moved against another build of the library.

Legs (B=128, T=50 unless changed):

* ``step``: the graph-replayed fused MOSI train step (``build_utt_fusion("mosi", embd_sizes=(w, w, w))``) for
  w = 64, 32, 128, warmed up (eager, capture, replays), then ``--steps`` replays each between its own pair of device
  events; the median, quartiles and extremes of the per-step device times go to the JSON.
* ``recurrence``: ``tspm_lstm_fwd`` / ``tspm_lstm_bwd`` (64) and ``tspm_lstm_fwd_w`` / ``tspm_lstm_bwd_w`` (32, 64, 128)
  through the C ABI on one LSTM with default-initialised weights, one launch between each pair of events.
* ``--ab-lib PATH``: the 64-wide step under the library at PATH (for instance the parent commit's, built with the
  Makefile's ``alt`` target) against this tree's, each in fresh child processes in alternating order, the other
  ``--ab-runs`` times each (5 by default; the range of the other library's medians is the measured spread):
  "within_spread" = the median of this tree's medians lies inside that range.  Every child also prints a checksum of
  the parameters, the loss and the logits after ``--check-steps`` seeded steps: the two libraries must agree bitwise
  ("outputs_bitwise_equal").  A library from
  before tspm_lstm_fwd_w lacks the two entry points; the child drops them from the signature table before loading it
  (the 64-wide step never calls them).

No default of the package depends on the result.  Needs the MI355X: there is no CPU leg.

    python scripts/bench_lstm_widths.py --out profiles/lstm_widths.json [--ab-lib path/to/libtspm_alt.so]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

WIDTHS = (64, 32, 128)


def summarise(us):
    q = statistics.quantiles(us, n=4)
    return {"median_us": statistics.median(us), "p25_us": q[0], "p75_us": q[2], "min_us": min(us), "max_us": max(us),
            "samples": len(us)}


def timed(fn, n):
    """n calls of fn, each between its own pair of device events → per-call device times in microseconds."""
    import torch
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]


def build_step(width, batch, steps, seed=3):
    import torch
    import tspm_amd
    from tspm_amd import mosi as M
    dev = torch.device("cuda", 0)
    c = M.YAML_CONFIGS["mosi"]
    torch.manual_seed(seed)
    kw = {} if width == 64 else {"embd_sizes": (width, width, width)}
    model = M.build_utt_fusion("mosi", **kw).to(dev)
    opt = tspm_amd.FusedAdam(model.parameters(), lr=c["lr"], weight_decay=c["weight_decay"])
    st = M.FusedMosiStep(model, opt, None, batch, steps)
    g = torch.Generator().manual_seed(1234)
    A = torch.randn(batch, steps, c["audio_dim"], generator=g).to(dev)
    V = (0.5 * torch.randn(batch, steps, c["video_dim"], generator=g)).to(dev)
    T = (0.3 * torch.randn(batch, steps, c["text_dim"], generator=g)).to(dev)
    y = torch.randint(0, 3, (batch,), generator=g).to(dev)
    st.eng.load(A, V, T, y)
    return model, st


def time_step(width, a):
    import math

    import torch
    model, st = build_step(width, a.batch, a.seq)
    for _ in range(a.warmup):  # eager, capture, replays
        st.run()
    torch.cuda.synchronize()
    if st.graph is None:
        raise SystemExit("bench_lstm_widths: the step was not captured (TSPM_NO_GRAPH set?)")
    if not math.isfinite(st.eng.loss.item()):
        raise SystemExit(f"width {width}: non-finite loss after warm-up")
    return summarise(timed(st.graph.replay, a.steps))


def checksum(a):
    """sha256 over the parameters and the loss after --check-steps seeded steps of the 64-wide step (device-drawn
    dropout masks from the model's seed: the same under any library that computes the same)."""
    import torch
    model, st = build_step(64, a.batch, a.seq)
    for _ in range(a.check_steps):
        st.run()
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for p in model.parameters():
        h.update(p.detach().cpu().numpy().tobytes())
    h.update(st.eng.loss.cpu().numpy().tobytes())
    h.update(st.eng.logits.cpu().numpy().tobytes())
    return h.hexdigest()


def time_recurrence(width, wide_entry, a):
    import torch
    from tspm_amd import _lib as L
    from tspm_amd import mosi as M
    dev = torch.device("cuda", 0)
    B, T, H = a.batch, a.seq, width
    torch.manual_seed(5)
    enc = M.LSTMEncoder(20, H, "last").to(dev)
    bufs = M._lstm_alloc(enc, B, T, dev)
    bufs["xg"].copy_(torch.randn(T * B, 4 * H, generator=torch.Generator().manual_seed(6)).to(dev))
    out, dh = torch.empty(B, H, device=dev), torch.randn(B, H, device=dev)
    f, b = (L.LstmFwdDesc * 1)(), (L.LstmBwdDesc * 1)()
    rnn = enc.rnn
    f[0].batch, f[0].steps, f[0].hidden, f[0].ld_out = B, T, H, H
    f[0].xg, f[0].w_hh, f[0].b_hh = bufs["xg"].data_ptr(), rnn.weight_hh_l0.data_ptr(), rnn.bias_hh_l0.data_ptr()
    f[0].gates, f[0].cs, f[0].hs, f[0].h_out = (bufs["gates"].data_ptr(), bufs["cs"].data_ptr(), bufs["hs"].data_ptr(),
                                                out.data_ptr())
    M._lstm_bwd_desc(b[0], enc, bufs, B, T, dh.data_ptr(), H)
    lib, sh = L.lib(), L.stream_handle()
    ff, fb = (lib.tspm_lstm_fwd_w, lib.tspm_lstm_bwd_w) if wide_entry else (lib.tspm_lstm_fwd, lib.tspm_lstm_bwd)
    res = {}
    for name, fn, d in (("fwd", ff, f), ("bwd", fb, b)):
        call = lambda: L.check(fn(1, d, sh), name)  # noqa: E731
        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        res[name] = summarise(timed(call, a.steps))
    return res


def child(a) -> None:
    """One fresh process under TSPM_LIB: the 64-wide step's time and checksum as one JSON line."""
    if a.legacy_lib:
        from tspm_amd import _lib as L
        for n in ("tspm_lstm_fwd_w", "tspm_lstm_bwd_w"):
            L._SIGS.pop(n, None)
    print("CHILD " + json.dumps({"step": time_step(64, a), "checksum": checksum(a)}), flush=True)


def run_child(lib_path, legacy, a):
    env = dict(os.environ)
    if lib_path:
        env["TSPM_LIB"] = lib_path
    else:
        env.pop("TSPM_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--batch", str(a.batch), "--seq", str(a.seq),
           "--steps", str(a.steps), "--warmup", str(a.warmup), "--check-steps", str(a.check_steps)]
    if legacy:
        cmd.append("--legacy-lib")
    out = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=600).stdout
    line = [ln for ln in out.splitlines() if ln.startswith("CHILD ")][-1]
    return json.loads(line[6:])


def lacks_wide_entry_points(path) -> bool:
    with open(path, "rb") as f:  # the export's name in the file (no second libtspm loaded into this process)
        return b"tspm_lstm_fwd_w" not in f.read()


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--seq", type=int, default=50)
    ap.add_argument("--steps", type=int, default=300, help="timed steps / launches per leg (the median is over these)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--check-steps", type=int, default=5)
    ap.add_argument("--ab-lib", default=None, help="another build of libtspm.so to compare the 64-wide step against")
    ap.add_argument("--ab-runs", type=int, default=5, help="fresh processes per library in the A/B leg")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--legacy-lib", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lstm_widths.json"))
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    result = {"batch": a.batch, "seq": a.seq, "timed_steps": a.steps,
              "timing": "one pair of device events per graph replay / per launch; median over the timed steps"}
    if a.ab_lib:  # children first: this process has not touched the GPU yet
        legacy = lacks_wide_entry_points(a.ab_lib)
        runs = {"other": [], "this": []}
        for which in ("other", "this") * a.ab_runs:
            runs[which].append(run_child(os.path.abspath(a.ab_lib) if which == "other" else None,
                                         legacy and which == "other", a))
            print(f"A/B {which}: {runs[which][-1]['step']['median_us']:.2f} us", flush=True)
        om = [r["step"]["median_us"] for r in runs["other"]]
        tm = [r["step"]["median_us"] for r in runs["this"]]
        sums = {r["checksum"] for rr in runs.values() for r in rr}
        result["ab_64"] = {"other_lib": os.path.basename(a.ab_lib), "other_medians_us": om, "this_medians_us": tm,
                           "other_spread_us": max(om) - min(om), "this_median_us": statistics.median(tm),
                           "within_spread": bool(min(om) <= statistics.median(tm) <= max(om)),
                           "outputs_bitwise_equal": len(sums) == 1, "runs": runs}
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_lstm_widths: needs the MI355X (no CPU leg)")
    result["device"] = torch.cuda.get_device_name(0)
    result["arch"] = torch.cuda.get_device_properties(0).gcnArchName
    result["step"] = {}
    for w in WIDTHS:
        result["step"][f"{w},{w},{w}"] = s = time_step(w, a)
        print(f"step widths ({w},{w},{w}): {s['median_us']:.2f} us [{s['p25_us']:.2f}, {s['p75_us']:.2f}]", flush=True)
    result["recurrence"] = {}
    for name, w, wide in (("64 (tspm_lstm_fwd/bwd)", 64, False), ("32", 32, True), ("64", 64, True), ("128", 128, True)):
        result["recurrence"][name] = r = time_recurrence(w, wide, a)
        print(f"recurrence {name}: fwd {r['fwd']['median_us']:.2f} us bwd {r['bwd']['median_us']:.2f} us", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out, "step_median_us": {k: round(v["median_us"], 2) for k, v in result["step"].items()},
                      "ab_64": {k: v for k, v in result.get("ab_64", {}).items() if k != "runs"}}))


if __name__ == "__main__":
    main()
