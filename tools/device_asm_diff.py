#!/usr/bin/env python3
"""Is the device code of two source trees the same?  `device_asm_diff.py TREE_A TREE_B [--profile] [--keep DIR]`.

Compiles every file of build.SOURCES in each tree to gfx950 assembly (build.FLAGS + --cuda-device-only -S), drops the
lines that carry `__hip_cuid_` (a per-file hash of the source text: the one expected difference) and compares the rest
as text.  A host-only change (entry points, argument checks, launch helpers) must come out `identical` for every file;
then kernel behaviour and kernel speed are unchanged by construction.  Needs hipcc only, no GPU.  Exit status 1 on a
difference."""
import argparse
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cavp_amd import build  # noqa: E402

JOBS = 16   # a fixed cap, not the CPU count: the compiles are memory-hungry and the box may be shared


def device_asm(tree, src, flags, out):
    cmd = [build._hipcc(), *flags, "--cuda-device-only", "-S", os.path.join(tree, "cavp_amd", "csrc", src), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed: " + " ".join(cmd) + "\n" + r.stderr)
    with open(out) as f:
        return [ln for ln in f if "__hip_cuid_" not in ln]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("--profile", action="store_true", help="compare the -DCAVP_PROFILE flavour")
    ap.add_argument("--keep", metavar="DIR", help="keep the .s files here (a/ and b/) instead of a temporary directory")
    args = ap.parse_args()
    flags = build.FLAGS + (["-DCAVP_PROFILE"] if args.profile else [])
    with tempfile.TemporaryDirectory() as tmp:
        root = args.keep or tmp
        jobs = {}
        with ThreadPoolExecutor(JOBS) as pool:
            for side, tree in (("a", args.tree_a), ("b", args.tree_b)):
                os.makedirs(os.path.join(root, side), exist_ok=True)
                for src in build.SOURCES:
                    out = os.path.join(root, side, src.replace(".hip", ".s"))
                    jobs[side, src] = pool.submit(device_asm, os.path.abspath(tree), src, flags, out)
        differ = 0
        for src in build.SOURCES:
            a, b = jobs["a", src].result(), jobs["b", src].result()
            differ += a != b
            print(f"{src:24s} {'identical' if a == b else 'DIFFERENT'}  ({len(a)} / {len(b)} lines)")
    print(f"{len(build.SOURCES) - differ} of {len(build.SOURCES)} identical" + (" (-DCAVP_PROFILE)" if args.profile else ""))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
