"""gic_xent next to gic_xent_seq doing the same job (no mask, eps = 0, w = 1) at the pre-training shape of cfg2 (rows = 64 * 20, V = 10 000),
f32 and bf16 logits, with and without the gradient, plus gic_xent_seq on a COCO-like padded batch (lengths ~11 of 20) for what the mask
saves.  One process; the two kernels alternate; every sample is --launches calls between two device events (400 calls of 20-50 us: a
window of 8-20 ms); the calls walk over --buffers distinct logits / gradient buffers (8 x 51 MB in f32: beyond the 256 MB Infinity
Cache), so the rows do come from HBM.  Bytes are counted from the shapes: gic_xent_seq reads the logits once and writes the gradient once
(its second read of a row is an L2 hit by construction and not counted); gic_xent's loops read a row twice (the max, then the sum of
exp; plus the one target logit, not counted) and once more for the gradient, which they write once: 2 rows V size without the
gradient, 4 with it (what reaches HBM of that is the hardware's business: the figure says how many bytes the kernel asks for).  The
time is that of the whole call between the events -- every launch of the entry point (gic_xent: 2, gic_xent_seq: 3) and the gaps
between them, not kernel time -- and so are the bytes per second and `hbm_share_of_call_time`, their share of the 6.3 TB/s a float4
copy reaches (the spec is 8.0).  Writes profiles/xent_seq_bench.json and prints one JSON line.
   python tools/xent_seq_bench.py [--repeats 9] [--launches 400] [--buffers 8]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BOUND = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--launches", type=int, default=400)
    ap.add_argument("--buffers", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xent_seq_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from gan_image_captioning_amd import _lib as L
    from gan_image_captioning_amd.engine import ptr, stream_ptr
    lib = L.load()
    dev = torch.device("cuda:0")
    B, Lc, V = 64, 20, 10000
    rows = B * Lc
    g = torch.Generator().manual_seed(1008)
    targets = torch.randint(3, V, (rows,), generator=g).to(dev)
    lengths = torch.randint(8, 15, (B,), generator=g, dtype=torch.int32).to(dev)            # COCO-like: ~11 of 20 positions
    counted = int(lengths.sum())
    loss_old = torch.empty(1 + rows, device=dev)
    loss_new, row_buf, cap_nll = torch.empty(2, device=dev), torch.empty(2, rows, device=dev), torch.empty(B, device=dev)
    cap_tokens = torch.empty(B, device=dev, dtype=torch.int32)
    out_rows = []
    for dtype, dt in ((torch.float32, L.F32), (torch.bfloat16, L.BF16)):
        xs = [(torch.randn(rows, V, generator=g) * 2.0).to(dtype).to(dev) for _ in range(a.buffers)]
        ds = [torch.empty_like(x) for x in xs]
        size = xs[0].element_size()
        for grad in (True, False):
            def old(i):
                L.check(lib.gic_xent(ptr(xs[i]), dt, rows, V, ptr(targets), ptr(loss_old), ptr(ds[i]) if grad else None, None, stream_ptr()))

            def new(i, masked=False):
                L.check(lib.gic_xent_seq(ptr(xs[i]), dt, rows, V, ptr(targets), Lc, ptr(lengths) if masked else None, -100, 0.0, None,
                                         ptr(loss_new), ptr(row_buf[0]), ptr(row_buf[1]), ptr(cap_nll), ptr(cap_tokens),
                                         ptr(ds[i]) if grad else None, stream_ptr()))
            kernels = {"gic_xent": (old, rows * V * size * (4 if grad else 2)),
                       "gic_xent_seq": (new, rows * V * size * (1 + (1 if grad else 0))),
                       "gic_xent_seq_masked": (lambda i: new(i, True), (counted + (rows if grad else 0)) * V * size)}
            us = {k: [] for k in kernels}
            for k, (fn, _) in kernels.items():            # warm-up: code objects, allocator, clocks
                for i in range(a.buffers):
                    fn(i)
            torch.cuda.synchronize()
            for _ in range(a.repeats):
                for k, (fn, _) in kernels.items():        # alternated: a drift of the clocks meets every kernel alike
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for j in range(a.launches):
                        fn(j % a.buffers)
                    e1.record()
                    e1.synchronize()
                    us[k].append(e0.elapsed_time(e1) * 1e3 / a.launches)
            for k, (_, nbytes) in kernels.items():
                med = statistics.median(us[k])
                out_rows.append({"kernel": k, "dtype": "f32" if dt == L.F32 else "bf16", "grad": grad, "rows": rows, "V": V,
                                 "us_median": round(med, 2), "us_min": round(min(us[k]), 2), "us_max": round(max(us[k]), 2),
                                 "bytes": nbytes, "tb_per_s": round(nbytes / med / 1e6, 3), "hbm_share_of_call_time": round(nbytes / med / 1e-6 / HBM_BOUND, 3)})
        del xs, ds
    res = {"what": "gic_xent vs gic_xent_seq, us per call (tools/xent_seq_bench.py)", "launches": a.launches, "repeats": a.repeats,
           "buffers": a.buffers, "hbm_bound_tb_per_s": HBM_BOUND / 1e12, "counted_rows_masked": counted, "rows": out_rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
