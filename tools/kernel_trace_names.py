#!/usr/bin/env python3
"""Reduce rocprofv3 kernel traces to the set of kernel instantiations that ran.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o NAME -- python -m pytest tests/test_gpu_X.py -m gpu
    python tools/kernel_trace_names.py [--all] [--out profiles/NAME.txt] [LABEL=]DIR/.../NAME_kernel_trace.csv ...

One section per trace: a "# LABEL" line (the path when no label is given), then one line "launches  kernel" per kernel of
the library, sorted by name, in the spelling of tests/kernel_variants.py (template arguments included, no namespace, no
argument list).  Kernels of other libraries (torch's own, rccl's) are left out unless --all is given.  Only the name column of
the trace is read.
"""
import argparse
import csv
import re
import subprocess
import sys
from collections import Counter

NAME_COLUMNS = ("Kernel_Name", "KernelName", "kernel_name", "Name")


def short_name(sym):
    """'void dvae::(anonymous namespace)::k_x<3, true>(float const*, int) [clone .kd]' -> ('k_x<3, true>', True); the flag says
    whether the kernel lives in namespace dvae."""
    s = sym.strip()
    if s.endswith(".kd"):
        s = s[:-3]
    s = s.replace("(anonymous namespace)::", "")
    depth, cut = 0, len(s)
    for i, ch in enumerate(s):              # the argument list opens at the first '(' outside template brackets
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            cut = i
            break
    s = s[:cut].strip()
    if s.startswith("void "):
        s = s[5:]
    ours = s.startswith("dvae::")
    if ours:
        s = s[len("dvae::"):]
    return s, ours


def demangle(names):
    """Itanium-mangled names through c++filt (one call); anything else is returned as it is."""
    todo = sorted({n for n in names if n.startswith("_Z")})
    if not todo:
        return {}
    try:
        out = subprocess.run(["c++filt"], input="\n".join(todo), capture_output=True, text=True, check=True).stdout.split("\n")
    except (OSError, subprocess.CalledProcessError):
        return {}
    return dict(zip(todo, out))


def reduce_trace(path, everything=False):
    """-> Counter {kernel: launches} of one kernel-trace CSV."""
    with open(path, newline="") as f:
        rd = csv.DictReader(f)
        col = next((c for c in NAME_COLUMNS if c in (rd.fieldnames or ())), None)
        if col is None:
            raise SystemExit("%s: no kernel-name column among %s" % (path, rd.fieldnames))
        raw = [row[col] for row in rd]
    dm = demangle(raw)
    seen = Counter()
    for n in raw:
        s, ours = short_name(dm.get(n.replace(".kd", ""), dm.get(n, n)))
        if ours or everything:
            seen[s] += 1
    return seen


def render(sections):
    lines = []
    for label, seen in sections:
        lines.append("# %s: %d kernels, %d launches" % (label, len(seen), sum(seen.values())))
        lines += ["%8d  %s" % (seen[k], k) for k in sorted(seen)]
    return "\n".join(lines) + "\n"


def split_label(arg):
    """'[LABEL=]PATH' -> (label, path): the label ends at the first '='; a left part with a '/' in it belongs to the path."""
    label, eq, path = arg.partition("=")
    if not eq or "/" in label or not label:
        return arg, arg
    return label, path


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("traces", nargs="+", help="[LABEL=]PATH of a *_kernel_trace.csv")
    ap.add_argument("--all", action="store_true", help="keep kernels outside namespace dvae")
    ap.add_argument("--out")
    a = ap.parse_args(argv)
    sections = []
    for t in a.traces:
        label, path = split_label(t)
        sections.append((label, reduce_trace(path, a.all)))
    text = render(sections)
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
