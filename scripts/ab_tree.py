#!/usr/bin/env python
"""A/B of two checkouts of this repository on the same box, each with its own built library: alternating ``bench.py``
processes (a fresh process per run, started inside its tree), same arguments, medians and ranges reported, and the last
step's outputs (``bench.py --dump-outputs``) of the two trees compared bit for bit.  ``scripts/ab_lib.py`` compares two
libraries under one Python tree; this compares a change that touches the Python side too against its parent commit
(``git archive <parent> | tar -x -C ab_old`` and ``make -C ab_old/<package>/csrc``; ``ab_old/`` is ignored by git).

    python scripts/ab_tree.py --b ab_old --rounds 3 --out profiles/avmnist_head_stage_ab.json -- --gpus 1 --steps 100 --warmup 20
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--a", default=REPO, help="tree A (this checkout)")
    ap.add_argument("--b", default=os.path.join(REPO, "ab_old"), help="tree B (the parent's checkout, built)")
    ap.add_argument("--out", default=None)
    ap.add_argument("rest", nargs=argparse.REMAINDER)
    a = ap.parse_args()
    rest = a.rest[1:] if a.rest and a.rest[0] == "--" else a.rest
    trees = {"A": os.path.abspath(a.a), "B": os.path.abspath(a.b)}
    res = {"A": [], "B": []}
    dumps = {}
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(a.rounds):
            for side in (("A", "B") if r % 2 == 0 else ("B", "A")):
                dump = os.path.join(tmp, f"{side}{r}")
                env = {k: v for k, v in os.environ.items() if k not in ("TSPM_LIB", "PYTHONPATH")}
                p = subprocess.run([sys.executable, "bench.py"] + rest + ["--dump-outputs", dump], cwd=trees[side],
                                   env=env, capture_output=True, text=True, timeout=400)
                if p.returncode != 0:
                    print(p.stderr[-3000:], file=sys.stderr)
                    raise SystemExit(f"{side} run failed ({p.returncode})")
                d = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
                res[side].append(d["ms_per_step"])
                dumps.setdefault(side, []).append(dump)
                print(f"round {r} {side}: {d['ms_per_step']:.4f} ms/step", file=sys.stderr, flush=True)
        names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(dumps["A"][0], "*.npy")))
        same = {}
        for n in names:
            blobs = [open(os.path.join(d, n), "rb").read() for side in ("A", "B") for d in dumps[side]]
            same[n] = all(b == blobs[0] for b in blobs)
    ms = {k: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v), "all": v} for k, v in res.items()}
    out = {"args": rest, "a": trees["A"], "b": trees["B"], "rounds": a.rounds, "ms_per_step": ms,
           "a_median_inside_b_range": ms["B"]["min"] <= ms["A"]["median"] <= ms["B"]["max"],
           "a_median_over_b_median": ms["A"]["median"] / ms["B"]["median"],
           "outputs_bitwise_equal": bool(names) and all(same.values()), "outputs": same}
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(out, a="this tree", b="the parent commit's tree"), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
