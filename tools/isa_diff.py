#!/usr/bin/env python3
"""Compare the gfx950 instruction streams of two source trees, file by file: the check a refactor of the kernels rests on.

    python tools/isa_diff.py OLD_TREE NEW_TREE [--variant product|stamps|nt ...] [--only conv3x3.hip ...] [--jobs N]

Every csrc/*.hip of both trees is compiled with build.py's FLAGS (NEW_TREE's build.py, with GIC_LIB_VARIANT set as for that library
variant) plus `--cuda-device-only -S`.  Comment lines, `.file`, `.ident` and the lines that carry the `__hip_cuid_<hash>` symbol (a
hash of the source text) are dropped; what is left must be equal.  Prints every file compared and, for a difference, its first
differing lines; exits 1 on any difference, or on a file that only one tree has.  No GPU is needed."""
from __future__ import annotations

import argparse
import concurrent.futures
import difflib
import glob
import importlib.util
import os
import subprocess
import sys
import tempfile

PKG = "gan-image-captioning_amd"
VARIANTS = {"product": "", "stamps": "stamps", "nt": "nt"}


def flags_of(tree: str, variant: str):
    """build.py's FLAGS and hipcc for one library variant (build.py reads GIC_LIB_VARIANT when it is imported)."""
    old = os.environ.get("GIC_LIB_VARIANT")
    os.environ["GIC_LIB_VARIANT"] = VARIANTS[variant]
    try:
        spec = importlib.util.spec_from_file_location(f"_gic_build_{variant}", os.path.join(tree, PKG, "build.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        if old is None:
            del os.environ["GIC_LIB_VARIANT"]
        else:
            os.environ["GIC_LIB_VARIANT"] = old
    return mod._hipcc(), list(mod.FLAGS)


def stream(hipcc: str, flags, src: str, out: str):
    r = subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", src, "-o", out], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed on {src}:\n{r.stdout}\n{r.stderr}")
    kept = []
    with open(out) as f:
        for line in f:
            s = line.strip()
            if not s or s.startswith(";") or s.startswith("//") or s.startswith(".file") or s.startswith(".ident") or "__hip_cuid_" in s:
                continue
            kept.append(line.rstrip())
    os.remove(out)
    return kept


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("--variant", nargs="+", choices=sorted(VARIANTS), default=["product", "stamps", "nt"])
    ap.add_argument("--only", nargs="+", default=None, help="file names under csrc/ (default: all *.hip)")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--lines", type=int, default=12, help="differing lines shown per file")
    a = ap.parse_args()

    def names(tree):
        return {os.path.basename(p) for p in glob.glob(os.path.join(tree, PKG, "csrc", "*.hip"))}

    old_names, new_names = names(a.old_tree), names(a.new_tree)
    todo = sorted(old_names | new_names)
    if a.only:
        todo = [n for n in todo if n in set(a.only)]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(max_workers=a.jobs) as ex:
        jobs = {}
        for variant in a.variant:
            hipcc, flags = flags_of(a.new_tree, variant)
            for n in todo:
                if n in old_names and n in new_names:
                    jobs[variant, n] = [ex.submit(stream, hipcc, flags, os.path.join(t, PKG, "csrc", n), os.path.join(tmp, f"{variant}.{side}.{n}.s"))
                                        for side, t in (("old", a.old_tree), ("new", a.new_tree))]
                else:
                    jobs[variant, n] = None
        for (variant, n), pair in jobs.items():
            if pair is None:
                print(f"{variant:8s} {n}: ONLY IN {'OLD' if n in old_names else 'NEW'} TREE")
                bad += 1
                continue
            old, new = pair[0].result(), pair[1].result()
            if old == new:
                print(f"{variant:8s} {n}: identical ({len(new)} lines)", flush=True)
                continue
            bad += 1
            print(f"{variant:8s} {n}: DIFFERENT ({len(old)} -> {len(new)} lines)")
            shown = 0
            for d in difflib.unified_diff(old, new, "old", "new", n=0, lineterm=""):
                if d.startswith(("---", "+++")):
                    continue
                print("    " + d)
                shown += 1
                if shown >= a.lines:
                    break
            sys.stdout.flush()
    print(f"{len(jobs) - bad} of {len(jobs)} comparisons identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
