#!/usr/bin/env python
"""What the UTT-Fusion head stage costs per step once the frozen encoders' outputs are cached.

The YAML models (MOSI: 64/64/64, MOSEI: BatchNorm1d classifier) with all three encoders frozen, synthetic data, at

  mosi_aligned     B = 128, steps 50
  mosi_unaligned   B = 128, steps (375, 500, 50)
  mosei_unaligned  B = 256, steps (500, 375, 50)

Legs, per shape (the baseline of every ratio is the uncached leg of the same process):

  step_frozen / cached_sample     (a) ``FusedMosiStep`` all-frozen against ``FusedMosiCachedStep(per_sample=True)``
  pattern_step / cached_every     (b) ``FusedMosiPatternStep`` all-frozen against ``FusedMosiCachedStep``, every pattern
  pattern_eval / cached_eval      (c) ``FusedMosiPatternEvalStep`` against ``FusedMosiCachedEvalStep``
  cache_rows                      (d) ``tspm_utt_cache_rows`` alone (halves = 2, with a mask), its own captured graph

and, wall clock: (e) the cache fill for ``--fill-rows`` rows (1,284 and 16,326) at the aligned MOSI and unaligned MOSEI
shapes, (f) a train epoch plus ``validate_epoch`` of ``EPOCH_BATCHES`` batches through ``MosiEpochRunner``, uncached
(``all_patterns`` / ``fuse_patterns`` loaders under a covering ``pad_to``) and cached (their ``ids_only`` twins).  The
cached step's launch count per replay is the library calls of one eager step.

Protocol: every leg of a shape is built and warmed up (eager, capture, replay) in this one process; then ``--runs``
rounds, each timing the legs one after the other (interleaved): ``--replays`` replays of the leg's captured graph, one
pair of device events per replay.  A round's figure is the median of its replays, a leg's the median of its round
medians, with their [min, max].  Needs the MI355X: there is no CPU leg.

    python scripts/bench_mosi_embedding_cache.py --out profiles/mosi_embedding_cache.json
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

SHAPES = {"mosi_aligned": ("mosi", 128, 50), "mosi_unaligned": ("mosi", 128, (375, 500, 50)),
          "mosei_unaligned": ("mosei", 256, (500, 375, 50))}
PAIRS = (("step_frozen", "cached_sample"), ("pattern_step", "cached_every"), ("pattern_eval", "cached_eval"))
ALL, EPOCH_BATCHES = ("audio", "video", "text"), 8


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


def build(name, dev, seed=0):
    import torch
    import tspm_amd
    from tspm_amd import mosi as M
    torch.manual_seed(seed)
    model = M.build_utt_fusion(name).to(dev)
    c = M.YAML_CONFIGS[name]
    opt = tspm_amd.FusedAdam(M.finetune_param_groups(model, lr=c["lr"], weight_decay=c["weight_decay"], freeze=ALL))
    return model, opt, c


def dataset(name, n, steps, dev, split="train", seed=1):
    from tspm_amd import mosi as M
    from tspm_amd.mosi_data import MOSI, synthetic_mosi_corpus
    c = M.YAML_CONFIGS[name]
    corpus = synthetic_mosi_corpus(n, seed=seed, steps=min(M.steps_triple(steps)),
                                   feats=(c["audio_dim"], c["video_dim"], c["text_dim"]))
    return MOSI(split=split, corpus=corpus, device=dev, seed=3)


class Recorder:
    """``_lib.lib()`` with every tspm_* call noted by name: the launch record of one eager step."""

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


def shape_legs(key, dev):
    """The legs of one shape, warmed up: {leg: callable replaying its captured graph}, and the launch counts."""
    import ctypes
    import torch
    from tspm_amd import _lib as L
    from tspm_amd import mosi as M
    from tspm_amd.metrics import ClassificationLog
    from tspm_amd.mosi_data import PATTERNS
    name, B, steps = SHAPES[key]
    ds = dataset(name, 4 * B, steps, dev)
    legs, counts = {}, {}
    # a captured graph holds raw pointers into its step's engine, model, optimizer and cache: everything a leg's graph
    # reads is kept alive here, next to the legs, for as long as the legs are replayed
    keep = legs["_keep"] = [ds]
    rows = torch.randperm(4 * B, device=dev)[:B].contiguous()
    Ts = M.steps_triple(steps)
    c = M.YAML_CONFIGS[name]
    A, V, T = (torch.randn(B, t, f, device=dev) for t, f in zip(Ts, (c["audio_dim"], c["video_dim"], c["text_dim"])))
    y = torch.randint(0, 3, (B,), device=dev)
    flags = torch.tensor([[int(ch in PATTERNS[i % 7]) for ch in "avt"] for i in range(B)], dtype=torch.uint8, device=dev)
    groups = (torch.arange(B, device=dev) % 7).to(torch.int32)
    keep.append((rows, A, V, T, y, flags, groups))

    def warm(leg, st, first):
        if leg.startswith("cached"):
            rec = Recorder(L.lib())
            real, L.lib = L.lib, (lambda: rec)
            try:
                first()
            finally:
                L.lib = real
            counts[leg] = {"library_calls": len(rec.calls), "calls": rec.calls}
        else:
            first()
        first()
        first()
        torch.cuda.synchronize()
        assert st.graph is not None
        legs[leg] = st.graph.replay

    for leg in ("step_frozen", "cached_sample", "pattern_step", "cached_every", "pattern_eval", "cached_eval"):
        model, opt, _ = build(name, dev)
        log = ClassificationLog(dev, groups=PATTERNS, classes=3)
        cached = leg.startswith("cached")
        cache = ds.embedding_cache(model, pad_to=steps) if cached else None
        if leg == "step_frozen":
            st = M.FusedMosiStep(model, opt, None, B, steps)
            st.eng.groups.copy_(groups)
            first = lambda st=st: st.step(A, V, T, y)  # noqa: E731
        elif leg == "cached_sample":
            st = M.FusedMosiCachedStep(model, opt, None, B, cache, per_sample=True)
            first = lambda st=st: st.step(rows, flags, groups)  # noqa: E731
        elif leg == "pattern_step":
            st = M.FusedMosiPatternStep(model, opt, None, B, steps)
            first = lambda st=st: st.step(A, V, T, y)  # noqa: E731
        elif leg == "cached_every":
            st = M.FusedMosiCachedStep(model, opt, None, B, cache)
            first = lambda st=st: st.step(rows)  # noqa: E731
        elif leg == "pattern_eval":
            st = M.FusedMosiPatternEvalStep(model, None, B, steps, log)
            first = lambda st=st: st.step(A, V, T, y)  # noqa: E731
        else:
            st = M.FusedMosiCachedEvalStep(model, None, B, cache, log)
            first = lambda st=st: st.step(rows)  # noqa: E731
        if not leg.endswith("eval"):
            st.log = log
        warm(leg, st, first)
        keep.append((st, model, opt, cache, log))
        if leg == "cached_every":  # (d): the cache read alone, as that step issues it
            e = st.eng.enc
            g = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with L.graph_capture(g):
                d = L.UttCacheRowsDesc(batch=B, halves=2, w_audio=cache.ha, w_video=cache.hv, w_pool=cache.nc,
                                       ld_cache=cache.W, ld_av=e.E, ld_pool=e.nc, n_rows=cache.n, n_zero=cache.n_zero,
                                       label_bytes=8, scale=2.0)
                d.emb, d.zero, d.rows = cache.emb.data_ptr(), cache.zero.data_ptr(), e.rows.data_ptr()
                d.labels_all, d.labels_out = cache.labels_all.data_ptr(), st.eng.labels.data_ptr()
                d.keep, d.av_out, d.pool_out = e.keeps[0].data_ptr(), e.fused.data_ptr(), e.fc_in.data_ptr()
                L.check(L.lib().tspm_utt_cache_rows(ctypes.byref(d), L.stream_handle()), "utt_cache_rows")
            legs["cache_rows"] = g.replay
            keep.append(g)
    return legs, counts


def epochs(key, dev, runs):
    """(f): a train epoch + validate_epoch of EPOCH_BATCHES batches, uncached and cached, wall clock: both runners are
    built and run once (build, capture), then ``runs`` rounds alternate the two legs; median and [min, max]."""
    import torch
    from tspm_amd import harness
    name, B, steps = SHAPES[key]
    out, legs = {}, {}
    for cached in (False, True):
        model, opt, _ = build(name, dev)
        tr, va = dataset(name, EPOCH_BATCHES * B, steps, dev), dataset(name, EPOCH_BATCHES * B, steps, dev, "valid", 2)
        lt = tr.loader(B, shuffle=True, seed=1, pad_to=steps, all_patterns=True, ids_only=cached)
        lv = va.loader(B, pad_to=steps, fuse_patterns=True, ids_only=cached)
        runner = harness.runner_for(model, opt, None)
        if cached:
            out["fill_seconds"] = {"train": tr.embedding_cache(model, pad_to=steps).fill_seconds,
                                   "validation": va.embedding_cache(model, pad_to=steps).fill_seconds}

        def one(runner=runner, lt=lt, lv=lv):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            runner.train_epoch(lt)
            runner.validate_epoch(lv)
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        one()
        one()  # the second pass captures
        legs["cached" if cached else "uncached"] = one
    rounds = {k: [] for k in legs}
    for _ in range(runs):
        for k, fn in legs.items():
            rounds[k].append(fn() * 1e3)
    out.update({k: spread(v, "ms") for k, v in rounds.items()})
    out["cached_entirely_below"] = out["cached"]["max_ms"] < out["uncached"]["min_ms"]
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--fill-rows", type=int, nargs="*", default=[1284, 16326])
    ap.add_argument("--no-epochs", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import tspm_amd  # noqa: F401
    dev = torch.device("cuda", 0)
    result = {"protocol": {"runs": args.runs, "replays": args.replays, "interleaved": True,
                           "timing": "one pair of device events per graph replay; round median, then median of rounds"},
              "shapes": {}}
    for key in args.shapes:
        legs, counts = shape_legs(key, dev)
        names = [k for k in legs if not k.startswith("_")]
        rounds = {k: [] for k in names}
        for _ in range(args.runs):
            for k in names:
                rounds[k].append(timed_calls(legs[k], args.replays))
        block = {"batch": SHAPES[key][1], "steps": SHAPES[key][2], "legs": {k: spread(v) for k, v in rounds.items()},
                 "launches": counts, "ratios": {}}
        for base, cached in PAIRS:
            b, c = block["legs"][base], block["legs"][cached]
            block["ratios"][f"{base}/{cached}"] = {"median": b["median_us"] / c["median_us"],
                                                   "cached_entirely_below": c["max_us"] < b["min_us"]}
        if not args.no_epochs:
            block["epoch"] = epochs(key, dev, args.runs)
        result["shapes"][key] = block
        print(json.dumps({key: {k: round(v["median_us"], 1) for k, v in block["legs"].items()}}), flush=True)
        del legs
    fills = {}
    for key in ("mosi_aligned", "mosei_unaligned"):
        if key not in args.shapes:
            continue
        name, B, steps = SHAPES[key]
        for n in args.fill_rows:
            model, _, _ = build(name, dev)
            ds = dataset(name, n, steps, dev)
            cache = ds.embedding_cache(model, pad_to=steps)
            first = cache.fill_seconds
            cache.refresh()
            fills[f"{key}/{n}"] = {"rows": n, "chunk": cache.chunk, "first_fill_s": first, "second_fill_s": cache.fill_seconds,
                                   "megabytes": cache.emb.numel() * 4 / 1e6}
            print(json.dumps({f"fill {key}/{n}": fills[f"{key}/{n}"]}), flush=True)
            del cache, ds, model
            torch.cuda.empty_cache()
    result["fill"] = fills
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({"written": args.out}))


if __name__ == "__main__":
    main()
