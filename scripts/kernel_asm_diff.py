#!/usr/bin/env python3
"""Per-kernel comparison of two gfx950 assembly files (``hipcc -O3 --offload-arch=gfx950 --cuda-device-only -S``).

    python scripts/kernel_asm_diff.py OLD.s NEW.s [--map OLD_SYMBOL_REGEX=NEW_SYMBOL_TEMPLATE ...] [--allow-kernarg]

For every kernel of OLD.s the kernel of NEW.s with the same symbol is looked up; ``--map`` renames old symbols first
(``re.sub`` on the whole mangled name, so one map with groups can cover a family of template instantiations; the first
map that matches is used).  Compared after normalisation — comments and blank lines dropped, the kernel's own symbol
and every other mangled symbol replaced by placeholders, basic-block labels renumbered in order of appearance:

  code        the instructions and labels between the kernel's entry label and its end
  descriptor  the ``.amdhsa_`` lines and the ``.set <symbol>.<resource>`` lines (register counts, LDS, scratch)
  metadata    the kernel's entry under ``amdhsa.kernels`` (register and spill counts, segment sizes) without ``.args``
  args        the ``.args`` list of that entry

Prints one line per kernel: ``same``, ``DIFF`` followed by the differing lines, or ``DIFF (kernel arguments only)`` when
nothing differs but the offsets of kernel-argument loads, the kernarg size and the argument list — what regrouping a
kernel's parameters produces.  Exit status 0 when every kernel is ``same`` (with ``--allow-kernarg``: or differs in its
kernel arguments only) and no kernel is missing on either side, else 1.  CPU only; it compares and nothing else.
"""
import argparse
import difflib
import re
import sys

SYM = re.compile(r"_Z\w+")
LABEL = re.compile(r"\.L(BB|func_end|func_begin|tmp|JTI)\d+(_\d+)?")
DROP = re.compile(r"^\.(section|globl|protected|weak|hidden|p2align|text|type|size)\b")
KERNARG_LOAD = re.compile(r"^(s_load_\w+\s+\S+\s+\S+\s+)(0x[0-9a-f]+|\d+)(.*)$")
KERNARG_KEY = re.compile(r"^(\.amdhsa_kernarg_size|\.kernarg_segment_size:)\s")


def strip(line):
    return line.split(";", 1)[0].strip()


def parse(path):
    """{symbol: {"code": [...], "descriptor": [...], "metadata": [...], "args": [...]}}"""
    lines = open(path).read().split("\n")
    kernels = {m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m}
    out = {k: {"code": [], "descriptor": [], "metadata": [], "args": []} for k in kernels}
    cur, part = None, None
    meta_at = next((i for i, l in enumerate(lines) if l.startswith("amdhsa.kernels:")), len(lines))
    for raw in lines[:meta_at]:
        l = strip(raw)
        m = re.match(r"\.type\s+(\S+),@function|\.amdhsa_kernel\s+(\S+)", l)
        if m:
            cur, part = m.group(1) or m.group(2), "code" if m.group(1) else "descriptor"
            continue
        m = re.match(r"\.set\s+(\S+)\.\w+,", l)
        if m and m.group(1) in kernels:
            out[m.group(1)]["descriptor"].append(l)
            continue
        if cur not in kernels or part is None or not l or l == cur + ":" or DROP.match(l):
            continue
        if l.startswith(".end_amdhsa_kernel"):
            part = None
            continue
        out[cur][part].append(l)
        if re.match(r"\.Lfunc_end\d+:", l):  # the kernel's code ends here
            part = None
    entries = []
    for raw in lines[meta_at + 1:]:
        if not raw.startswith("  "):
            break
        if raw.startswith("  - "):
            entries.append([])
        entries[-1].append(raw)
    for e in entries:
        name = next((l.split(":", 1)[1].strip() for l in e if l.startswith("    .name:")), None)  # the kernel's, not an argument's
        if name not in out:
            continue
        in_args = False
        for raw in e:
            body = raw[4:]
            if body.startswith(".args:"):
                in_args = True
                continue
            if in_args and body.startswith(" "):
                out[name]["args"].append(body.strip())
                continue
            in_args = False
            out[name]["metadata"].append(body.strip())
    return out


def normalise(lines, own):
    labels = {}

    def label(m):
        return labels.setdefault(m.group(0), ".L%s#%d" % (m.group(1), len(labels)))

    def sym(m):
        s = m.group(0)
        return "<kernel>" + s[len(own):] if s.startswith(own) else "<symbol>"

    return [LABEL.sub(label, SYM.sub(sym, l)) for l in lines]


def mask_kernarg(line):
    m = KERNARG_LOAD.match(line)
    if m:
        return m.group(1) + "<offset>" + m.group(3)
    return KERNARG_KEY.sub(lambda k: k.group(1) + " <size>", line)


def compare(old, new, old_sym, new_sym):
    """(differing lines, True when they are confined to the kernel arguments)"""
    report, only_args = [], True
    for part in ("code", "descriptor", "metadata", "args"):
        a, b = normalise(old[part], old_sym), normalise(new[part], new_sym)
        if a == b:
            continue
        diff = [d for d in difflib.unified_diff(a, b, "old", "new", lineterm="", n=0) if not d.startswith(("---", "+++"))]
        report += ["  [%s]" % part] + ["    " + d for d in diff]
        if part != "args" and [mask_kernarg(l) for l in a] != [mask_kernarg(l) for l in b]:
            only_args = False
    return report, only_args


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--map", action="append", default=[], metavar="OLD_REGEX=NEW_TEMPLATE")
    ap.add_argument("--allow-kernarg", action="store_true", help="differences in the kernel arguments alone do not fail")
    a = ap.parse_args()
    maps = [(re.compile(m.split("=", 1)[0]), m.split("=", 1)[1]) for m in a.map]
    old, new = parse(a.old), parse(a.new)
    bad, seen = 0, set()
    for k in sorted(old):
        target = next((rx.sub(t, k) for rx, t in maps if rx.fullmatch(k)), k)
        if target not in new:
            print("MISSING in new: %s (looked for %s)" % (k, target))
            bad += 1
            continue
        seen.add(target)
        report, only_args = compare(old[k], new[target], k, target)
        name = k if k == target else "%s -> %s" % (k, target)
        if not report:
            print("same  %s (%d lines)" % (name, len(old[k]["code"])))
        else:
            print("DIFF%s  %s" % (" (kernel arguments only)" if only_args else "", name))
            print("\n".join(report))
            bad += not (only_args and a.allow_kernarg)
    for k in sorted(set(new) - seen):
        print("MISSING in old: %s" % k)
        bad += 1
    print("%d kernels compared, %d not accepted" % (len(old), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
