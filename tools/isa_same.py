"""Do two csrc trees compile to the same device code?  For a change that moves
kernel source between headers and must leave the machine code alone.

    git worktree add ../parent <commit>
    python tools/isa_same.py ../parent [--branch .] [--out profiles/isa_same.json]

Every unit of tools/build_native.py's HIP_SOURCES that both trees have (a unit
one tree lacks is listed under "only_in" and not compared) is compiled to gfx950
assembly from both trees (hipcc --cuda-device-only -S, the build's flags) and
compared function by function: the instruction lines and the labels between
them, comments and assembler directives dropped, basic-block labels renumbered
per function (.LBB<function>_<block>: the function's number is its place in the
unit).  The verdict per kernel -- its name, identical or not, the instruction
count on each side -- goes to --out; the exit status is 1 if any differs.
It only diffs; it looks for no instruction in particular.
"""
from __future__ import annotations

import argparse
import json
import os
import re
import shutil
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import build_native as B   # noqa: E402


def functions(asm: str) -> dict:
    """name -> (is a kernel, its lines) of every function in a unit's assembly."""
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    out, name, lines = {}, None, []
    types = set(re.findall(r"^\s*\.type\s+(\S+),@function", asm, re.M))
    for raw in asm.splitlines():
        line = raw.split(";", 1)[0].strip()
        if not line:
            continue
        if name is None:
            if line.endswith(":") and line[:-1] in types:
                name, lines = line[:-1], []
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = (name in kernels, lines)
            name = None
        elif line.endswith(":") or not line.startswith("."):   # a label or an instruction
            lines.append(re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", line))
    return out


def assembly(tree: str, unit: str, tmp: str, tag: str) -> str:
    csrc, include = os.path.join(tree, "ocljpegdecoder_amd", "csrc"), os.path.join(tree, "include")
    flags = [f for f in B.COMMON if not f.startswith("-I")] + [f"-I{include}", f"-I{csrc}"]
    out = os.path.join(tmp, f"{tag}_{unit}.s")
    B._run([B.HIPCC, f"--offload-arch={B.ARCH}", "--cuda-device-only", "-S", *flags, os.path.join(csrc, unit), "-o", out])
    with open(out) as f:
        return f.read()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent", help="the other tree (a checkout of the commit to compare with)")
    ap.add_argument("--branch", default=REPO)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "isa_same.json"))
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--units", help="comma-separated units of HIP_SOURCES (default: all)")
    ap.add_argument("--keep", help="a directory to leave the assembly files in (to diff what differs)")
    args = ap.parse_args()
    sources = args.units.split(",") if args.units else B.HIP_SOURCES
    trees = {"parent": os.path.abspath(args.parent), "branch": os.path.abspath(args.branch)}
    has = {tag: [u for u in sources if os.path.exists(os.path.join(tree, "ocljpegdecoder_amd", "csrc", u))]
           for tag, tree in trees.items()}
    only_in = {tag: [u for u in has[tag] if u not in has[other]] for tag, other in (("parent", "branch"), ("branch", "parent"))}
    sources = [u for u in sources if u in has["parent"] and u in has["branch"]]
    tmp = args.keep or tempfile.mkdtemp(prefix="isa_same_")
    os.makedirs(tmp, exist_ok=True)
    try:
        jobs = [(tag, unit) for unit in sources for tag in trees]
        with ThreadPoolExecutor(max_workers=args.jobs) as ex:
            asms = dict(zip(jobs, ex.map(lambda j: functions(assembly(trees[j[0]], j[1], tmp, j[0])), jobs)))
    finally:
        if not args.keep:
            shutil.rmtree(tmp, ignore_errors=True)
    units, differ = {}, 0
    for unit in sources:
        p, b = asms[("parent", unit)], asms[("branch", unit)]
        rows = []
        for n in sorted(set(p) | set(b)):
            (pk, pl), (bk, bl) = p.get(n, (False, None)), b.get(n, (False, None))
            count = [None if x is None else sum(not ln.endswith(":") for ln in x) for x in (pl, bl)]
            rows.append({"name": n, "kernel": pk or bk, "identical": pl == bl, "instructions_parent": count[0],
                         "instructions_branch": count[1]})
            differ += pl != bl
        units[unit] = {"functions": len(rows), "identical": all(r["identical"] for r in rows), "kernels": rows}
    result = {"what": "device assembly of every HIP unit, parent tree against branch tree, function by function "
                      "(instructions and labels; comments and directives dropped)",
              "arch": B.ARCH, "flags": [f for f in B.COMMON if not f.startswith("-I")],
              "functions": sum(u["functions"] for u in units.values()), "differ": differ, "only_in": only_in,
              "units": units}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"isa_same": "ok" if not differ else "differ", "functions": result["functions"], "differ": differ,
                      "file": os.path.relpath(args.out, REPO)}))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
