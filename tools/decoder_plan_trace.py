#!/usr/bin/env python3
"""The decoder passes' launch sequence, for comparing two trees: one eager call per path, a separator kernel between them.

    rocprofv3 --kernel-trace --mangled-kernels --output-format csv -d OUT -- python tools/decoder_plan_trace.py run
    python tools/decoder_plan_trace.py rows OUT/**/*_kernel_trace.csv > trace.txt

`run` makes the calls below on cuda:0 (kernel trace alone: no counters, no other tracing); `rows` turns the trace into one line per
launch -- kernel with its template arguments (read off the mangled name), Grid_Size X x Y in work-items, Workgroup_Size X -- with a
`phase N` line where the separator (a torch cos_ on 3 floats) ran.  Two trees launch the same kernels iff their `rows` files are equal
(profiles/decoder_plan_trace.txt: the commit before selection and launch were separated in the decoder passes).

Phases, bf16, cfg2's decoder (V = 10000, E = H = 512, NL = 1, L = 20) unless noted:
  1  sample_fwd + sample_bwd, B = 64 (fused step kernels)            2  the same at V = 9998 (generic products)
  3  ids-only sample_fwd, B = 520 (row keys, Gumbel-max epilogue)    4  resumed roll-out: B = 8, L = 6, 14 roll-outs per prefix, 560 rows
  5  forward_tf + forward_tf_bwd, B = 64                             6  forward_scheduled, B = 64      7  the same at V = 9998
  8  AttnDecoderEngine.rollout: B = 4, L = 5, V = 1280, E = 16, H = 32, C = 40, P = 49, A = 24, 121 roll-outs per prefix (484 .. 1936
     rows per step: the last one is past the 1921 from which the vocabulary product carries the Gumbel-max)
  9  beam_search, B = 4, beam 3, L = 6                               10 the same at V = 9998"""
import csv
import re
import sys


def run():
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from gan_image_captioning_amd import _lib, engine as E
    from oracle import cpu_attention as A
    from oracle import cpu_step as O
    from tests.gpu_util import dec_param_names
    dev = torch.device("cuda:0")
    mark = torch.zeros(3, device=dev)
    g = torch.Generator().manual_seed(7)

    def lstm(V, Em=512, H=512):
        gp = O.make_gen_params(V, Em, H, 1, g)
        return E.DecoderEngine(V, Em, H, 1, _lib.BF16), [gp[n].to(dev) for n in dec_param_names(1)]

    def feats(B, Em=512):
        return (torch.randn(B, Em, generator=g) * 0.3).to(dev)

    def phase():
        torch.cuda.synchronize()
        mark.cos_()

    for V in (10000, 9998):                                    # 1, 2
        dec, params = lstm(V)
        dec.prepare(params)
        phase()
        out, ids, st = dec.sample_fwd(params, feats(64), 20, 0.9, seed=1)
        dec.sample_bwd(params, st, out, ids, torch.ones_like(out), 0.9)
    dec, params = lstm(10000)
    dec.prepare(params)
    phase()                                                    # 3
    dec.sample_fwd(params, feats(520), 20, 1.0, seed=2, ids_only=True)
    B, L, N = 8, 6, 14
    f = feats(B)
    _, Y, _ = dec.sample_fwd(params, f, L, 1.0, seed=3, ids_only=True)
    reps = (L - 1) * N
    flen = torch.arange(1, L, device=dev, dtype=torch.int32).repeat_interleave(N * B)
    _, _, st_y = dec.sample_fwd(params, f, L, 1.0, pretrain=True, force_ids=Y)
    phase()                                                    # 4
    dec.sample_fwd(params, f.repeat(reps, 1), L, 1.0, seed=4, ids_only=True, force_ids=Y.repeat(reps, 1), force_len=flen,
                   resume=(st_y, B, [min(t, L - 1) * N * B for t in range(L)]))
    caps = torch.randint(3, 9000, (64, 20), generator=g).to(dev)
    f = feats(64)
    phase()                                                    # 5
    pred, _, saved = dec.forward_tf(params, f, caps, [21] * 64, 1.0, pretrain=True, keep_state=True)
    dec.forward_tf_bwd(params, saved, pred, torch.ones_like(pred), 1.0, pretrain=True)
    for V in (10000, 9998):                                    # 6, 7
        dec, params = lstm(V)
        dec.prepare(params)
        phase()
        dec.forward_scheduled(params, f, caps, [21] * 64, 0.25, seed=5)
    B, L, V, Em, H, C, P, At, N = 4, 5, 1280, 16, 32, 40, 49, 24, 121
    gp = {k: v * 6.0 for k, v in A.make_attn_params(V, Em, H, C, At, g).items()}
    names = ["decoder.embed.weight", "decoder.lstm.weight_ih_l0", "decoder.lstm.weight_hh_l0", "decoder.lstm.bias_ih_l0", "decoder.lstm.bias_hh_l0",
             "decoder.linear.weight", "decoder.linear.bias", "decoder.attn.w_f", "decoder.attn.b_f", "decoder.attn.w_h", "decoder.attn.w_a"]
    att = E.AttnDecoderEngine(V, Em, H, C, P, At, _lib.BF16)
    ap = [gp[n].to(dev).contiguous() for n in names]
    fa, fmap = feats(B, Em), torch.relu(torch.randn(B, P, C, generator=g)).to(dev)
    _, Y, _ = att.sample_fwd(ap, fa, fmap, L, 1.0, seed=6)
    saved = att.forward_tf(ap, fa, fmap, Y[:, :-1], [L] * B, 1.0, pretrain=True, keep_state=True)[3]
    phase()                                                    # 8
    att.rollout(ap, saved, Y, N, seed=7)
    for V in (10000, 9998):                                    # 9, 10
        dec, params = lstm(V)
        dec.prepare(params)
        f = feats(4)
        phase()
        dec.beam_search(params, f, 6, 3)
    phase()
    torch.cuda.synchronize()


def short(m):
    """`_ZN3gic12_GLOBAL__N_120lstm_bwd_step_kernelIDF16bLi8EEEvNS_15LstmBwdStepArgsE` -> `lstm_bwd_step_kernel<bf16,8>`: the mangled names
    (rocprofv3 --mangled-kernels; its demangler garbles the bf16 type and the arguments behind it), as far as this library's kernels need"""
    def ident(i):                                              # <length><identifier>
        j = i
        while m[j].isdigit():
            j += 1
        n = int(m[i:j])
        return m[j:j + n], j + n

    def nested(i):                                             # N ... E: the last component
        last = ""
        while m[i] != "E":
            if m[i] == "S":                                    # a substitution: S_ | S<seq>_
                i = m.index("_", i) + 1
            elif m[i] == "I":
                _, i = targs(i + 1)
            else:
                last, i = ident(i)
        return last, i + 1

    def targs(i):                                              # behind the I: ... E
        out = []
        while m[i] != "E":
            if m.startswith("DF16b", i):
                out.append("bf16"); i += 5
            elif m[i] == "L":                                  # L <type> <value> E
                t, j = m[i + 1], m.index("E", i)
                v = m[i + 2:j].replace("n", "-")
                out.append({"0": "false", "1": "true"}[v] if t == "b" else v); i = j + 1
            elif m[i] == "N":
                t, i = nested(i + 1); out.append(t)
            elif m[i].isdigit():
                t, i = ident(i); out.append(t)
            else:
                out.append({"f": "f32", "i": "int", "h": "u8", "b": "bool"}[m[i]]); i += 1
        return out, i + 1

    try:
        if m.startswith("_ZN"):
            i, name = 3, ""
            while m[i] not in "EI":
                name, i = ident(i)
        elif m.startswith("_Z"):
            name, i = ident(2)
        else:
            return m
        return name + ("<" + ",".join(targs(i + 1)[0]) + ">" if m[i] == "I" else "")
    except (KeyError, ValueError, IndexError):
        return m


def rows(paths):
    recs = []
    for p in paths:
        with open(p, newline="") as f:
            recs += list(csv.DictReader(f))
    recs.sort(key=lambda r: int(r["Start_Timestamp"]))
    n = 0
    for r in recs:
        k = r["Kernel_Name"]
        if "cos_kernel" in k and "elementwise" in k:
            n += 1
            print(f"phase {n}")
        elif n and "2at6native" not in k and not k.startswith("__amd_rocclr"):      # (torch's own kernels and the runtime's fills / copies)
            print(f"{short(k)}  {r['Grid_Size_X']}x{r['Grid_Size_Y']}  {r['Workgroup_Size_X']}")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) > 2 and sys.argv[1] == "rows":
        rows(sys.argv[2:])
    else:
        sys.exit(__doc__)
