#!/usr/bin/env python
"""Unaligned MOSI / MOSEI on the UTT-Fusion HIP path: what the fused train step and the two LSTM recurrences cost when
audio, video and text run at their own lengths, next to the aligned length 50 at the same batch, and whether the aligned
step moved against another build of the library.

Shapes (Ta, Tv, Tt):

* ``mosi``:  (375, 500, 50), B = 128 — ``build_utt_fusion("mosi")``, embedding "last" (no time index);
* ``mosei``: (500, 375, 50), B = 256 — ``build_utt_fusion("mosei")``, embedding "maxpool": both recurrences take the
  16-bit time index (tspm_lstm_fwd_t16 / tspm_lstm_bwd_t16);
* ``*_aligned``: 50 steps for every modality at the same batch.

Legs:

* ``step``: the graph-replayed fused train step, warmed up (eager, capture, replays), then ``--steps`` replays
  (``--long-steps`` for the unaligned shapes) each between its own pair of device events; median, quartiles, extremes.
* ``recurrence``: the step's own two-encoder launches alone — ``_lib.lstm_fwd`` / ``_lib.lstm_bwd`` on the engine's
  buffers after a step has filled them — one launch between each pair of events.
* ``--ab-lib PATH``: the aligned MOSI step (B = 128, T = 50) under the library at PATH (for instance the parent commit's)
  against this tree's, in fresh child processes in alternating order, ``--ab-runs`` each (5 by default):
  "within_range" = the median of this tree's medians lies inside the other library's own min–max range.  Every child
  also prints a checksum of the parameters, loss and logits after ``--check-steps`` seeded steps; the two libraries
  must agree bitwise.  A library from before the 16-bit or the per-sample-length entry points lacks them; the child
  drops the exports its library file does not have from the signature table before loading it (the aligned step never
  calls them).

Nothing in the package depends on the result.  Needs the MI355X: there is no CPU leg.

    python scripts/bench_mosi_unaligned.py --out profiles/mosi_unaligned.json [--ab-lib path/to/other/libtspm.so]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import math
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SHAPES = {"mosi_aligned": ("mosi", 128, 50), "mosi": ("mosi", 128, (375, 500, 50)),
          "mosei_aligned": ("mosei", 256, 50), "mosei": ("mosei", 256, (500, 375, 50))}
T16 = ("tspm_lstm_fwd_t16", "tspm_lstm_bwd_t16")
LATER = T16 + ("tspm_lstm_fwd_len", "tspm_lstm_bwd_len", "tspm_textcnn_pool_fwd_len", "tspm_adam_begin_multi",
               "tspm_adam_step_multi", "tspm_grad_clip_coef_multi", "tspm_lstm_bwd_seq", "tspm_attn_pool_fwd",
               "tspm_attn_pool_bwd")  # exports an older build of the library may lack


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


def build_step(name, batch, steps, seed=3):
    import torch
    import tspm_amd
    from tspm_amd import mosi as M
    dev = torch.device("cuda", 0)
    c = M.YAML_CONFIGS[name]
    torch.manual_seed(seed)
    model = M.build_utt_fusion(name).to(dev)
    opt = tspm_amd.FusedAdam(model.parameters(), lr=c["lr"], weight_decay=c["weight_decay"])
    st = M.FusedMosiStep(model, opt, None, batch, steps)
    ta, tv, tt = M.steps_triple(steps)
    g = torch.Generator().manual_seed(1234)
    A = torch.randn(batch, ta, c["audio_dim"], generator=g).to(dev)
    V = (0.5 * torch.randn(batch, tv, c["video_dim"], generator=g)).to(dev)
    T = (0.3 * torch.randn(batch, tt, c["text_dim"], generator=g)).to(dev)
    y = torch.randint(0, 3, (batch,), generator=g).to(dev)
    st.eng.load(A, V, T, y)
    return model, st


def time_shape(key, a):
    """→ {"step": ..., "recurrence": {"fwd": ..., "bwd": ...}} of one shape."""
    import torch
    from tspm_amd import _lib as L
    from tspm_amd import mosi as M
    name, batch, steps = SHAPES[key]
    n = a.steps if isinstance(steps, int) else a.long_steps
    model, st = build_step(name, batch, steps)
    for _ in range(a.warmup):  # eager, capture, replays
        st.run()
    torch.cuda.synchronize()
    if st.graph is None:
        raise SystemExit("bench_mosi_unaligned: the step was not captured (TSPM_NO_GRAPH set?)")
    if not math.isfinite(st.eng.loss.item()):
        raise SystemExit(f"{key}: non-finite loss after warm-up")
    out = {"model": name, "batch": batch, "steps": list(M.steps_triple(steps)), "wide_index": bool(st.eng.wide),
           "step": summarise(timed(st.graph.replay, n))}
    # the recurrences alone, as the step launches them: both encoders in one call, on the buffers the step filled
    e, m, sh = st.eng, model, L.stream_handle()
    ta, tv, _ = e.Ts
    fd, bd = (L.LstmFwdDesc * 2)(), (L.LstmBwdDesc * 2)()
    for i, (nm, enc, x, col, t) in enumerate((("a", m.netA, e.A, 0, ta), ("v", m.netV, e.V, m.netA.hidden_size, tv))):
        M._lstm_fwd_prepare(fd[i], enc, x, e.lstm[nm], batch, t, e.fused.data_ptr() + col * 4, e.E, sh)
        M._lstm_bwd_desc(bd[i], enc, e.lstm[nm], batch, t, e.dfused.data_ptr() + col * 4, e.E)
    out["recurrence"] = {}
    for leg, call in (("fwd", lambda: L.check(L.lstm_fwd(2, fd, sh, e.wide), "lstm_fwd")),
                      ("bwd", lambda: L.check(L.lstm_bwd(2, bd, sh, e.wide), "lstm_bwd"))):
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        out["recurrence"][leg] = summarise(timed(call, n))
    return out


def checksum(a):
    """sha256 over the parameters, the loss and the logits after --check-steps seeded aligned MOSI steps."""
    import torch
    model, st = build_step(*SHAPES["mosi_aligned"])
    for _ in range(a.check_steps):
        st.run()
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for p in model.parameters():
        h.update(p.detach().cpu().numpy().tobytes())
    h.update(st.eng.loss.cpu().numpy().tobytes())
    h.update(st.eng.logits.cpu().numpy().tobytes())
    return h.hexdigest()


def child(a) -> None:
    """One fresh process under TSPM_LIB: the aligned MOSI step's time and checksum as one JSON line."""
    if a.legacy_lib:
        from tspm_amd import _lib as L
        for n in missing_exports(L.LIB_PATH):
            L._SIGS.pop(n, None)
    print("CHILD " + json.dumps({"step": time_shape("mosi_aligned", a)["step"], "checksum": checksum(a)}), flush=True)


def run_child(lib_path, legacy, a):
    env = dict(os.environ)
    if lib_path:
        env["TSPM_LIB"] = lib_path
    else:
        env.pop("TSPM_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--steps", str(a.steps), "--long-steps",
           str(a.long_steps), "--warmup", str(a.warmup), "--check-steps", str(a.check_steps)]
    if legacy:
        cmd.append("--legacy-lib")
    out = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=300).stdout
    return json.loads([ln for ln in out.splitlines() if ln.startswith("CHILD ")][-1][6:])


def missing_exports(path):
    with open(path, "rb") as f:  # the exports' names in the file (no second libtspm loaded into this process)
        blob = f.read()
    return [n for n in LATER if n.encode() + b"\0" not in blob]


def lacks_t16(path) -> bool:
    return T16[0] in missing_exports(path)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=300, help="timed replays / launches at the aligned shapes")
    ap.add_argument("--long-steps", type=int, default=40, help="timed replays / launches at the unaligned shapes")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--check-steps", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES), help="comma-separated subset of: " + ", ".join(SHAPES))
    ap.add_argument("--ab-lib", default=None, help="another build of libtspm.so to compare the aligned step against")
    ap.add_argument("--ab-runs", type=int, default=5, help="fresh processes per library in the A/B leg")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--legacy-lib", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mosi_unaligned.json"))
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    result = {"timing": "one pair of device events per graph replay / per launch; median over the timed samples"}
    if a.ab_lib:  # children first: this process has not touched the GPU yet
        legacy = bool(missing_exports(a.ab_lib))
        runs = {"other": [], "this": []}
        for which in ("other", "this") * a.ab_runs:
            runs[which].append(run_child(os.path.abspath(a.ab_lib) if which == "other" else None,
                                         legacy and which == "other", a))
            print(f"A/B {which}: {runs[which][-1]['step']['median_us']:.2f} us", flush=True)
        om = [r["step"]["median_us"] for r in runs["other"]]
        tm = [r["step"]["median_us"] for r in runs["this"]]
        sums = {r["checksum"] for rr in runs.values() for r in rr}
        result["ab_aligned"] = {"shape": "mosi B=128 T=50", "other_lib": os.path.basename(a.ab_lib),
                                "other_medians_us": om, "this_medians_us": tm, "other_min_us": min(om),
                                "other_max_us": max(om), "other_median_us": statistics.median(om),
                                "this_median_us": statistics.median(tm),
                                "within_range": bool(min(om) <= statistics.median(tm) <= max(om)),
                                "outputs_bitwise_equal": len(sums) == 1, "runs": runs}
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mosi_unaligned: needs the MI355X (no CPU leg)")
    result["device"] = torch.cuda.get_device_name(0)
    result["arch"] = torch.cuda.get_device_properties(0).gcnArchName
    result["shapes"] = {}
    for key in [k for k in a.shapes.split(",") if k]:
        result["shapes"][key] = r = time_shape(key, a)
        print(f"{key} {tuple(r['steps'])} B={r['batch']}: step {r['step']['median_us']:.1f} us "
              f"[{r['step']['min_us']:.1f}, {r['step']['max_us']:.1f}]  recurrence fwd "
              f"{r['recurrence']['fwd']['median_us']:.1f} us bwd {r['recurrence']['bwd']['median_us']:.1f} us", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out, "ab_aligned": {k: v for k, v in result.get("ab_aligned", {}).items() if k != "runs"}}))


if __name__ == "__main__":
    main()
