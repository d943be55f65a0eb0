#!/usr/bin/env python3
"""No GPU needed: is the device code of two trees the same, kernel by kernel?

    python tools/isa_identity.py PARENT_TREE [--out profiles/NAME.txt] [--work DIR] [--jobs N] [--builds shipped,debug]

PARENT_TREE is a checkout of the commit to compare against (e.g. `git worktree add /tmp/parent HEAD~1`).  Every source of
every target in build.py's TARGETS table is compiled to device-only assembly in both trees with the project's flags, once
plain and once with -DDVAE_DEBUG_SWITCHES.  Comments and assembler directives are stripped; what is left (labels + instructions) is compared per
function, together with each kernel's .vgpr_count / .sgpr_count / .private_segment_fixed_size / .group_segment_fixed_size
and the "; Occupancy:" comment.  Prints one line per file and build, and for every kernel that differs the resource lines
of both sides.  Exit status 1 when anything differs.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "disentangling-vae_amd"
sys.path.insert(0, os.path.join(ROOT, PKG))
import build as dvae_build  # noqa: E402

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--offload-device-only", "-S"]
ALL_SOURCES = dvae_build.ALL_SOURCES
META = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def compile_s(tree, stem, extra, out):
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + FLAGS + extra + [os.path.join(tree, PKG, "csrc", stem + ".hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed: %s\n%s" % (" ".join(cmd), r.stderr))


def parse(path):
    """-> ({function: [label / instruction lines]}, {kernel: {resource: value}})"""
    code, res, recs, cur, last = {}, {}, [], None, None
    for line in open(path):
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            cur = last = m.group(1)
            code[cur] = []
            continue
        m = re.match(r"\s*; Occupancy: (\d+)", line)                # in the comment block behind the function's end
        if m and last:
            res.setdefault(last, {})["occupancy"] = m.group(1)
        if re.match(r"\s*- \.agpr_count:", line):                   # a kernel's .amdgpu_metadata record opens with this key
            recs.append({})
        m = re.match(r"\s*\.symbol:\s+(\S+)\.kd", line)
        if m and recs:
            recs[-1]["name"] = m.group(1)
        m = re.match(r"\s*(\.\w+):\s+(\d+)\s*$", line)
        if m and m.group(1) in META and recs:
            recs[-1][m.group(1)] = m.group(2)
        text = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0].strip())     # block labels carry the function's ordinal in the file
        if cur and text.startswith(".Lfunc_end"):
            cur = None
        elif cur and text and (not text.startswith(".") or text.endswith(":")):      # directives go, local labels stay
            code[cur].append(text)
    for r in recs:
        res.setdefault(r.pop("name"), {}).update(r)
    return code, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("--out")
    ap.add_argument("--work")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--builds", default="shipped,debug", help="fc_chain.hip takes minutes with the debug switches")
    a = ap.parse_args()
    work = a.work or tempfile.mkdtemp(prefix="isa_identity_")
    trees = {"parent": os.path.abspath(a.parent), "tip": ROOT}
    builds = {b: ["-DDVAE_DEBUG_SWITCHES"] if b == "debug" else [] for b in a.builds.split(",")}
    jobs = []
    for side, tree in trees.items():
        for b, extra in builds.items():
            os.makedirs(os.path.join(work, side, b), exist_ok=True)
            for s in ALL_SOURCES:
                out = os.path.join(work, side, b, s + ".s")
                if side == "tip" or not os.path.exists(out):       # a parent already compiled into --work is kept
                    jobs.append((tree, s, extra, out))
    with ThreadPoolExecutor(max_workers=a.jobs) as ex:
        list(ex.map(lambda j: compile_s(*j), jobs))

    lines, differ = [], 0
    for b in builds:
        for s in ALL_SOURCES:
            pc, pr = parse(os.path.join(work, "parent", b, s + ".s"))
            tc, tr = parse(os.path.join(work, "tip", b, s + ".s"))
            bad = [f for f in sorted(set(pc) | set(tc)) if pc.get(f) != tc.get(f) or pr.get(f) != tr.get(f)]
            n_ins = sum(len(v) for v in tc.values())
            lines.append("%-8s %-18s %-9s %3d functions %6d lines" % (b, s + ".hip", "DIFFERS" if bad else "identical", len(tc), n_ins))
            for f in bad:
                differ += 1
                lines.append("    %s: %d -> %d lines" % (f, len(pc.get(f, [])), len(tc.get(f, []))))
                lines.append("        parent %s" % sorted(pr.get(f, {}).items()))
                lines.append("        tip    %s" % sorted(tr.get(f, {}).items()))
    lines.append("%d function(s) differ" % differ)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
