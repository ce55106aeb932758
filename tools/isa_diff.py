#!/usr/bin/env python3
"""Compare the gfx950 instruction streams of two source trees, file by file: the check a refactor of the kernels rests on.

    python tools/isa_diff.py OLD_TREE NEW_TREE [--variant product|stamps|nt ...] [--only conv3x3.hip ...] [--jobs N] [--by-kernel]

Every csrc/*.hip of both trees is compiled with build.py's FLAGS (NEW_TREE's build.py, with GIC_LIB_VARIANT set as for that library
variant) plus `--cuda-device-only -S`.  Comment lines, `.file`, `.ident` and the lines that carry the `__hip_cuid_<hash>` symbol (a
hash of the source text) are dropped; what is left must be equal.  Prints every file compared and, for a difference, its first
differing lines; exits 1 on any difference, or on a file that only one tree has.  No GPU is needed.

--by-kernel: for a refactor that cannot keep a whole file's stream (a helper shared between kernels moves the scheduler's choices), each
file's stream is split at its kernel symbols and every kernel gets one status: `identical`, `only in old`, `only in new` or `changed`.
A changed kernel is printed with the resources the compiler records for it in the kernel metadata (vector + accumulator registers and
the waves per SIMD that they and a static LDS array leave -- a dynamic LDS request is not in the metadata and not counted --, scratch
bytes, LDS bytes) and its instruction counts by family, old -> new.  The families are a
classification of every mnemonic by its prefix (FAMILIES); `kept` marks a changed kernel whose scratch, LDS and occupancy are unchanged
and whose matrix / LDS / vector-memory / s_waitcnt / s_barrier counts are equal, `REVIEW` any other.  Exits 1 on a kernel only one tree
has or marked REVIEW."""
from __future__ import annotations

import argparse
import concurrent.futures
import difflib
import glob
import importlib.util
import os
import re
import shutil
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


# ---------------------------------------------------------------------------------------------- --by-kernel
# every instruction belongs to the first family whose prefix its mnemonic starts with
FAMILIES = (("matrix", ("v_mfma",)), ("lds", ("ds_",)), ("vmem", ("buffer_", "global_", "flat_", "scratch_")), ("waitcnt", ("s_waitcnt",)),
            ("barrier", ("s_barrier",)), ("vector", ("v_",)), ("scalar", ("s_",)))
PINNED = ("matrix", "lds", "vmem", "waitcnt", "barrier")          # the families a `kept` kernel may not change
RESOURCES = (("vgpr", ".vgpr_count"), ("agpr", ".agpr_count"), ("scratch", ".private_segment_fixed_size"), ("lds", ".group_segment_fixed_size"),
             ("block", ".max_flat_workgroup_size"))
_FUNC_INDEX = re.compile(r"\.(LBB|Lfunc_begin|Lfunc_end|LJTI|Ltmp)\d+")


def family_of(mnemonic: str) -> str:
    for name, prefixes in FAMILIES:
        if mnemonic.startswith(prefixes):
            return name
    return "other"


def count_families(lines):
    """Instruction counts by family of one kernel's lines (labels and directives are no instructions)."""
    counts = {name: 0 for name, _ in FAMILIES}
    counts["other"] = 0
    for line in lines:
        s = line.strip()
        if not s or s.startswith((".", ";")) or s.split(";")[0].strip().endswith(":"):
            continue
        counts[family_of(s.split()[0])] += 1
    return counts


def split_kernels(lines):
    """{kernel symbol: its lines from the label to the end of the function}, for the symbols that `.amdhsa_kernel` names.  The
    function's index in the file is taken out of its local labels (.LBB<index>_<n>) and trailing comments are dropped (the loop notes name
    BB<index>_<n> too): a kernel does not change because one above it left."""
    names = {l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel")}
    out, cur = {}, None
    for line in lines:
        s = line.strip()
        if cur is None:
            head = s.split(";")[0].strip()
            if head.endswith(":") and head[:-1] in names:
                cur = head[:-1]
                out[cur] = []
            continue
        if s.startswith(".Lfunc_end"):
            cur = None
            continue
        out[cur].append(_FUNC_INDEX.sub(lambda m: "." + m.group(1), line.split(";")[0].rstrip()))
    return out


def kernel_resources(lines):
    """{kernel symbol: {vgpr, agpr, scratch, lds, block}} from the kernel metadata (the YAML between .amdgpu_metadata and .end_amdgpu_metadata)."""
    out, entry, inside = {}, None, False
    keys = {key: name for name, key in RESOURCES}

    def close():
        if entry and ".name" in entry:
            out[entry[".name"]] = {name: int(entry.get(key, 0)) for name, key in RESOURCES}

    for line in lines:
        s = line.strip()
        if s == ".amdgpu_metadata":
            inside = True
        elif s == ".end_amdgpu_metadata":
            inside = False
        elif inside:
            top = line.startswith("    .")                    # a key of the kernel itself (its argument list is indented deeper)
            if line.startswith("  - "):                       # the next kernel of amdhsa.kernels
                close()
                entry, top = {}, True
                s = s[2:].strip()
            if entry is not None and top and ":" in s:
                key, val = s.split(":", 1)
                if key in keys or key == ".name":
                    entry[key] = val.strip()
    close()
    return out


def waves_per_simd(res) -> int:
    """Occupancy the unified register file leaves (512 registers per lane and SIMD, allocated in granules of 8, at most 8 waves) and,
    where the kernel has a static LDS array, the workgroups that fit a CU's 160 KiB, as waves on each of its 4 SIMDs.  Dynamic LDS is the
    launch's, not the kernel's (group_segment_fixed_size is 0 for the dynamic-LDS convolution kernels): for those this is the occupancy
    the registers allow, and what their LDS request leaves is the host's select_* to keep (tests/test_route.py pins the lds= figures)."""
    total = (res["vgpr"] + 3) // 4 * 4 + res["agpr"]
    waves = min(8, 512 // max(8, (total + 7) // 8 * 8))
    if res["lds"] and res["block"]:
        waves = min(waves, (160 * 1024 // res["lds"]) * ((res["block"] + 63) // 64) // 4)
    return waves


def compare_kernels(old_lines, new_lines):
    """[(symbol, status, detail lines)] over the kernels of both streams; status: identical | only in old | only in new | kept | REVIEW."""
    ok, nk = split_kernels(old_lines), split_kernels(new_lines)
    ores, nres = kernel_resources(old_lines), kernel_resources(new_lines)
    rows = []
    for name in sorted(set(ok) | set(nk)):
        if name not in nk or name not in ok:
            rows.append((name, "only in old" if name in ok else "only in new", []))
        elif ok[name] == nk[name]:
            rows.append((name, "identical", []))
        else:
            ro, rn = ores.get(name), nres.get(name)
            co, cn = count_families(ok[name]), count_families(nk[name])
            good = all(co[f] == cn[f] for f in PINNED)
            detail = []
            if ro and rn:
                good = good and ro["scratch"] == rn["scratch"] and ro["lds"] == rn["lds"] and waves_per_simd(ro) == waves_per_simd(rn)
                detail.append("    " + "  ".join(f"{k} {ro[k]} -> {rn[k]}" for k, _ in RESOURCES[:4]) + f"  waves/SIMD {waves_per_simd(ro)} -> {waves_per_simd(rn)}")
            else:
                good = False
                detail.append("    (no kernel metadata)")
            detail.append("    " + "  ".join(f"{f} {co[f]} -> {cn[f]}" for f in co if co[f] or cn[f]))
            rows.append((name, "kept" if good else "REVIEW", detail))
    return rows


def demangler():
    exe = shutil.which("llvm-cxxfilt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    if not os.path.exists(exe):
        return lambda names: names
    return lambda names: subprocess.run([exe], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")[:len(names)] if names else []


def report_by_kernel(variant, n, old, new, demangle) -> int:
    rows = compare_kernels(old, new)
    tally = {}
    for _, status, _ in rows:
        tally[status] = tally.get(status, 0) + 1
    print(f"{variant:8s} {n}: " + (", ".join(f"{v} {k}" for k, v in sorted(tally.items())) or "no kernels"), flush=True)
    shown = [r for r in rows if r[1] != "identical"]
    for (name, status, detail), pretty in zip(shown, demangle([r[0] for r in shown])):
        print(f"  {'changed, ' + status if status in ('kept', 'REVIEW') else status}: {pretty}")
        for d in detail:
            print(d)
    return sum(1 for _, status, _ in rows if status not in ("identical", "kept"))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("--variant", nargs="+", choices=sorted(VARIANTS), default=["product", "stamps", "nt"])
    ap.add_argument("--only", nargs="+", default=None, help="file names under csrc/ (default: all *.hip)")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--lines", type=int, default=12, help="differing lines shown per file")
    ap.add_argument("--by-kernel", action="store_true", help="one status per kernel instead of one per file (see above)")
    a = ap.parse_args()

    def names(tree):
        return {os.path.basename(p) for p in glob.glob(os.path.join(tree, PKG, "csrc", "*.hip"))}

    old_names, new_names = names(a.old_tree), names(a.new_tree)
    todo = sorted(old_names | new_names)
    if a.only:
        todo = [n for n in todo if n in set(a.only)]
    bad = 0
    demangle = demangler()
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
            if a.by_kernel:
                bad += 1 if report_by_kernel(variant, n, old, new, demangle) else 0
                continue
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
    print(f"{len(jobs) - bad} of {len(jobs)} comparisons " + ("within the rule" if a.by_kernel else "identical"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
