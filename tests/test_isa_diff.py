"""tools/isa_diff.py --by-kernel: the splitter of an assembly stream at its kernel symbols, the kernel-metadata reader and the
instruction counter by mnemonic family, on a few lines of synthetic assembly (no compiler, no GPU)."""
import importlib.util
import os

_spec = importlib.util.spec_from_file_location("isa_diff", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "isa_diff.py"))
isa_diff = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa_diff)


def asm(kernels):
    """A stream as isa_diff.stream() leaves it (no comment lines): `kernels` = [(symbol, body lines, vgpr, agpr, scratch, lds)], each as
    function number i of the file (in its labels and in the compiler's loop note behind a label), with a device function that is no
    kernel ahead of them."""
    out = ["\t.text", "helper:", "\tv_mov_b32_e32 v0, 0", "\ts_setpc_b64 s[30:31]", ".Lfunc_end0:"]
    meta = ["\t.amdgpu_metadata", "---", "amdhsa.kernels:"]
    for i, (name, body, vgpr, agpr, scratch, lds) in enumerate(kernels, start=1):
        out += [f"\t.globl\t{name}", f"{name}:                                 ; @{name}"]
        out += [b.replace("LBB_", f".LBB{i}_") + (f"              ;   in Loop: Header=BB{i}_1 Depth=1" if b.endswith(":") else "") for b in body]
        out += [f".Lfunc_end{i}:", f"\t.size\t{name}, .Lfunc_end{i}-{name}", f"\t.amdhsa_kernel {name}", "\t\t.amdhsa_next_free_vgpr 8", "\t.end_amdhsa_kernel"]
        meta += [f"  - .agpr_count:     {agpr}", "    .args:", "      - .name:           d", "        .offset:         0", "        .size:           8",
                 f"    .group_segment_fixed_size: {lds}", "    .max_flat_workgroup_size: 256", f"    .name:           {name}",
                 f"    .private_segment_fixed_size: {scratch}", f"    .symbol:         {name}.kd", f"    .vgpr_count:     {vgpr}"]
    return out + meta + ["amdhsa.target:   amdgcn-amd-amdhsa--gfx950", "...", "\t.end_amdgpu_metadata"]


BODY = ["\ts_load_dwordx2 s[0:1], s[4:5], 0x0", "\ts_waitcnt lgkmcnt(0)", "LBB_1:", "\tglobal_load_dwordx4 v[0:3], v4, s[0:1]",
        "\tbuffer_load_dwordx4 v5, s[8:11], 0 offen lds", "\ts_waitcnt vmcnt(0)", "\ts_barrier", "\tds_read_b128 v[8:11], v6",
        "\tv_mfma_f32_16x16x32_bf16 v[12:15], v[0:3], v[8:11], v[12:15]", "\tv_add_u32_e32 v4, 16, v4", "\ts_cbranch_scc1 LBB_1",
        "\tscratch_load_dword v4, off, off", "\tflat_store_dword v[0:1], v4", "\ts_endpgm"]


def test_families_classify_by_prefix():
    counts = isa_diff.count_families(BODY)
    assert counts == {"matrix": 1, "lds": 1, "vmem": 4, "waitcnt": 2, "barrier": 1, "vector": 1, "scalar": 3, "other": 0}
    assert isa_diff.family_of("v_mfma_f32_32x32x16_bf16") == "matrix" and isa_diff.family_of("v_accvgpr_write_b32") == "vector"
    assert isa_diff.family_of("s_waitcnt_vscnt") == "waitcnt" and isa_diff.family_of("exp") == "other"
    assert isa_diff.count_families(["LBB_1:", "\t.p2align\t8", "k:      ; @k"]) == dict.fromkeys(counts, 0)     # labels, directives: none


def test_split_takes_kernels_only_and_drops_the_function_index():
    k = isa_diff.split_kernels(asm([("ka", BODY, 16, 0, 0, 1024), ("kb", BODY[:2] + ["\ts_endpgm"], 8, 4, 0, 0)]))
    assert sorted(k) == ["ka", "kb"]                                       # `helper` is no kernel
    assert len(k["ka"]) == len(BODY) and len(k["kb"]) == 3
    assert ".LBB_1:" in k["ka"] and "\ts_cbranch_scc1 .LBB_1" in k["ka"]
    # the same kernel as function 1 of one file and function 2 of another is the same stream
    moved = isa_diff.split_kernels(asm([("other", ["\ts_endpgm"], 8, 0, 0, 0), ("ka", BODY, 16, 0, 0, 1024)]))
    assert moved["ka"] == k["ka"]


def test_resources_come_from_the_kernel_metadata():
    res = isa_diff.kernel_resources(asm([("ka", BODY, 100, 28, 0, 65536), ("kb", BODY, 8, 4, 16, 0)]))
    assert res["ka"] == {"vgpr": 100, "agpr": 28, "scratch": 0, "lds": 65536, "block": 256}
    assert res["kb"] == {"vgpr": 8, "agpr": 4, "scratch": 16, "lds": 0, "block": 256}
    assert isa_diff.waves_per_simd(res["kb"]) == 8
    assert isa_diff.waves_per_simd({"vgpr": 100, "agpr": 28, "scratch": 0, "lds": 0, "block": 256}) == 4        # 128 registers
    assert isa_diff.waves_per_simd(res["ka"]) == 2                          # two 64 KiB workgroups of 4 waves per CU


def test_statuses():
    old = asm([("same", BODY, 16, 0, 0, 0), ("gone", BODY, 16, 0, 0, 0), ("renamed_regs", BODY, 16, 0, 0, 0), ("spills", BODY, 16, 0, 0, 0),
               ("extra_load", BODY, 16, 0, 0, 0)])
    new = asm([("added", BODY, 16, 0, 0, 0), ("same", BODY, 16, 0, 0, 0),
               ("renamed_regs", [b.replace("v4", "v7") for b in BODY] + ["\ts_nop 0"], 17, 0, 0, 0),
               ("spills", [b.replace("v4", "v7") for b in BODY], 16, 0, 8, 0),
               ("extra_load", BODY[:4] + ["\tglobal_load_dword v9, v4, s[0:1]"] + BODY[4:], 16, 0, 0, 0)])
    rows = {name: (status, detail) for name, status, detail in isa_diff.compare_kernels(old, new)}
    assert {n: s for n, (s, _) in rows.items()} == {"same": "identical", "gone": "only in old", "added": "only in new", "renamed_regs": "kept",
                                                    "spills": "REVIEW", "extra_load": "REVIEW"}
    assert "vgpr 16 -> 17" in rows["renamed_regs"][1][0] and "scalar 3 -> 4" in rows["renamed_regs"][1][1]
    assert "scratch 0 -> 8" in rows["spills"][1][0]
    assert "vmem 4 -> 5" in rows["extra_load"][1][1]
