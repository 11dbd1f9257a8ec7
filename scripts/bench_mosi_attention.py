#!/usr/bin/env python
"""What the attention embedding of the LSTM encoders costs on the UTT-Fusion HIP path: the fused train step with
``LSTMEncoder(embd_method="attention", attention_norm="time" | "unit")`` next to the step as the YAML builds it ("last" for
MOSI, "maxpool" for MOSEI), and the added launches on their own.

Shapes (Ta, Tv, Tt): MOSI aligned 50 at B = 128, MOSI (375, 500, 50) at B = 128, MOSEI (500, 375, 50) at B = 256.

Protocol (DESIGN §3.12's): every leg's step is built and warmed up (eager, capture, replays) once; then ``--runs`` rounds
(5), each timing the legs one after the other (interleaved), ``--steps`` graph replays per leg and round (``--long-steps``
at the unaligned shapes), each replay between its own pair of device events; a leg's figure is the median of its round
medians, with their range.  ``calls``: the libtspm calls of one eager step (input gathers and workspace queries left out;
tspm_attn_pool_bwd and the split-K weight gradients are two kernels each).  ``added``: the new calls alone — and the
recurrence calls they follow — timed one by one between device events on an eager step with the side stream off
(``MosiEngine.concurrent = False``), median over ``--steps`` steps; eager launches of a few microseconds include the
launch gaps, so these say where the time goes, not what the graph saves.

Nothing in the package depends on the result.  Needs the MI355X: there is no CPU leg.

    python scripts/bench_mosi_attention.py --out profiles/mosi_attention.json
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

SHAPES = {"mosi_aligned": ("mosi", 128, 50), "mosi": ("mosi", 128, (375, 500, 50)), "mosei": ("mosei", 256, (500, 375, 50))}
LEGS = ("as_built", "time", "unit")
RECURRENCES = ("tspm_lstm_fwd", "tspm_lstm_bwd", "tspm_lstm_fwd_w", "tspm_lstm_bwd_w", "tspm_lstm_fwd_t16", "tspm_lstm_bwd_t16",
               "tspm_lstm_fwd_len", "tspm_lstm_bwd_len", "tspm_lstm_bwd_seq")
NEW = ("tspm_attn_pool_fwd", "tspm_attn_pool_bwd", "tspm_linear_bwd_data")


def build_step(name, batch, steps, leg, seed=3):
    import torch
    import tspm_amd
    from tspm_amd import mosi as M
    dev = torch.device("cuda", 0)
    c = M.YAML_CONFIGS[name]
    torch.manual_seed(seed)
    kw = {} if leg == "as_built" else dict(embd_method="attention", attention_norm=leg)
    model = M.build_utt_fusion(name, **kw).to(dev)
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


class _Proxy:
    """``L.lib()`` with every tspm_* call noted; with ``events`` set, the watched calls run between device events."""

    def __init__(self, lib, hidden):
        self._lib, self.calls, self.events, self.hidden = lib, [], None, hidden

    def _label(self, name, args):
        if name in RECURRENCES or name in NEW:
            return name
        h = self.hidden
        if name == "tspm_linear_fwd" and args[1] == args[2] == h and args[0] > 4096:
            return "tspm_linear_fwd (attention projection)"
        if name == "tspm_linear_bwd_weight_splitk" and args[1] == args[2] == h:
            return "tspm_linear_bwd_weight_splitk (attention dW)"
        return None

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("tspm_"):
            return fn

        def call(*args):
            import torch
            self.calls.append(name)
            label = self._label(name, args) if self.events is not None else None
            if label is None:
                return fn(*args)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*args)
            e1.record()
            self.events.append((label, e0, e1))
            return rc
        return call


def replay_medians(st, n):
    import torch
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for e0, e1 in ev:
        e0.record()
        st.graph.replay()
        e1.record()
    torch.cuda.synchronize()
    return statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)


def time_shape(key, a):
    import torch
    from tspm_amd import _lib as L
    name, batch, steps = SHAPES[key]
    n = a.steps if isinstance(steps, int) else a.long_steps
    real = L.lib()
    legs = {}
    for leg in LEGS:
        proxy = _Proxy(real, 64)
        L.lib = lambda p=proxy: p
        model, st = build_step(name, batch, steps, leg)
        st.run()  # eager: the call record
        torch.cuda.synchronize()
        calls = [c for c in proxy.calls if not c.endswith("_workspace") and c != "tspm_seq_gather"]
        # the watched calls one by one, on eager forward + loss + backward with the side stream off
        st.eng.concurrent, proxy.events = False, []
        for _ in range(n):
            st._fwd_bwd()
        torch.cuda.synchronize()
        per = {}
        for label, e0, e1 in proxy.events:
            per.setdefault(label, []).append(e0.elapsed_time(e1) * 1e3)
        added = {k: {"median_us": statistics.median(v), "per_step": len(v) // n} for k, v in per.items()}
        st.eng.concurrent, proxy.events = True, None
        L.lib = lambda: real
        for _ in range(a.warmup):  # capture, replays
            st.run()
        torch.cuda.synchronize()
        if st.graph is None or not math.isfinite(st.eng.loss.item()):
            raise SystemExit(f"{key} {leg}: the step was not captured or its loss is not finite")
        legs[leg] = dict(st=st, model=model, calls=len(calls), new_calls=sorted(set(calls) & set(NEW + ("tspm_lstm_bwd_seq",))),
                         added=added, rounds=[])
    for _ in range(a.runs):  # interleaved
        for leg in LEGS:
            legs[leg]["rounds"].append(replay_medians(legs[leg]["st"], n))
    out = {"model": name, "batch": batch, "steps": list(steps) if not isinstance(steps, int) else [steps] * 3, "replays": n,
           "legs": {}}
    base = statistics.median(legs["as_built"]["rounds"])
    for leg in LEGS:
        r = legs[leg]["rounds"]
        out["legs"][leg] = {"step_median_us": statistics.median(r), "round_medians_us": r, "min_us": min(r), "max_us": max(r),
                            "ratio_to_as_built": statistics.median(r) / base, "calls": legs[leg]["calls"],
                            "new_calls": legs[leg]["new_calls"], "added": legs[leg]["added"]}
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200, help="timed replays per leg and round at the aligned shape")
    ap.add_argument("--long-steps", type=int, default=40, help="... at the unaligned shapes")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mosi_attention.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mosi_attention: needs the MI355X (no CPU leg)")
    result = {"timing": "one pair of device events per graph replay; a leg = the median of its round medians; rounds interleave "
                        "the legs", "device": torch.cuda.get_device_name(0),
              "arch": torch.cuda.get_device_properties(0).gcnArchName, "runs": a.runs, "shapes": {}}
    for key in [k for k in a.shapes.split(",") if k]:
        result["shapes"][key] = r = time_shape(key, a)
        print(key, {leg: (round(v["step_median_us"], 1), v["calls"]) for leg, v in r["legs"].items()}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
