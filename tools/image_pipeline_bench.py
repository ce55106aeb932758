"""gic_image_preprocess at the loader's shape: B = 64 images of 480 x 640 x 3 -> 224 x 224 (whole image, no flip), next to the host work
it replaces.

Device: every sample is --launches calls between two device events, walking over --buffers distinct (pixels, output) pairs (6 x 59 MB
+ 6 x 38.5 MB: beyond the 256 MB Infinity Cache, so the bytes come from HBM).  The time is that of the whole call -- the descriptor
staging launch (one per 64 images) and the kernel -- not kernel time alone.  Byte floor: the source bytes read once plus the output
written once over the 6.3 TB/s a float4 copy reaches on this part (the spec is 8.0); a row band re-reads the
source rows it shares with its neighbours, which the floor does not count (L2 / Infinity Cache absorb most of it).

Host: the arithmetic of tasks.load_image on already-decoded arrays (PIL resize to S x S, f32, / 255, normalise, transpose), the same
64 images spread over --procs worker processes (started before the parent touches the GPU), median wall time of --host-repeats
rounds.  JPEG decoding is in neither number, and the end-to-end loader throughput is not measured here.

Also the bytes uploaded per batch on either path.  Writes profiles/image_pipeline_bench.json and prints one JSON line.
   python tools/image_pipeline_bench.py [--repeats 9] [--launches 50] [--buffers 6] [--procs 16]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BOUND = 6.3e12
B, H, W, S = 64, 480, 640, 224


def _host_one(seed):
    import numpy as np
    from PIL import Image
    arr = _HOST_IMAGES[seed % len(_HOST_IMAGES)]
    mean = np.array([0.485, 0.456, 0.406], dtype=np.float32)
    std = np.array([0.229, 0.224, 0.225], dtype=np.float32)
    im = Image.fromarray(arr).resize((S, S), resample=Image.BILINEAR)
    out = (np.asarray(im, dtype=np.float32) / 255.0 - mean) / std
    return float(np.ascontiguousarray(out.transpose(2, 0, 1))[0, 0, 0])


_HOST_IMAGES = []


def host_time(procs, repeats):
    """Median seconds for B images through load_image's arithmetic on ``procs`` processes; None without PIL or with --procs 0."""
    if procs <= 0:
        return None
    try:
        import PIL  # noqa: F401
    except ImportError:
        return None
    import multiprocessing as mp
    import numpy as np
    rng = np.random.RandomState(0)
    _HOST_IMAGES.extend(rng.randint(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(8))
    times = []
    with mp.get_context("fork").Pool(procs) as pool:
        pool.map(_host_one, range(B))                       # warm-up: imports, page faults
        for _ in range(repeats):
            t0 = time.perf_counter()
            pool.map(_host_one, range(B), chunksize=max(1, B // procs))
            times.append(time.perf_counter() - t0)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--buffers", type=int, default=6)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--host-repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_pipeline_bench.json"))
    a = ap.parse_args()
    host_s = host_time(a.procs, a.host_repeats)             # before the GPU is opened: the workers never see it
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from gan_image_captioning_amd import engine
    from gan_image_captioning_amd.tasks import RawImageBatch
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(1)
    batches = [RawImageBatch.from_arrays([rng.randint(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(B)], S) for _ in range(a.buffers)]
    src = engine.image_srcs(batches[0].descs())
    pixels = [b.pixels.to(dev) for b in batches]
    outs = [torch.empty(B, 3, S, S, device=dev) for _ in range(a.buffers)]
    read_bytes, write_bytes = B * H * W * 3, B * 3 * S * S * 4

    def call(i):
        engine.image_preprocess(pixels[i], src, S, out=outs[i])
    for i in range(a.buffers):                               # warm-up: code object, allocator, clocks
        call(i)
    torch.cuda.synchronize()
    us = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for j in range(a.launches):
            call(j % a.buffers)
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / a.launches)
    med = statistics.median(us)
    floor_us = (read_bytes + write_bytes) / HBM_BOUND * 1e6
    res = {"what": "gic_image_preprocess, B = 64 of 480x640x3 -> 224 (tools/image_pipeline_bench.py)", "launches": a.launches,
           "repeats": a.repeats, "buffers": a.buffers, "call_us_median": round(med, 2), "call_us_min": round(min(us), 2),
           "call_us_max": round(max(us), 2), "bytes_read": read_bytes, "bytes_written": write_bytes, "hbm_bound_tb_per_s": HBM_BOUND / 1e12,
           "byte_floor_us": round(floor_us, 2), "floor_share_of_call_time": round(floor_us / med, 3),
           "images_per_s_device": round(B / med * 1e6), "host_procs": a.procs,
           "host_ms_median": None if host_s is None else round(host_s * 1e3, 2),
           "images_per_s_host": None if host_s is None else round(B / host_s),
           "upload_bytes_device_path": int(batches[0].pixels.numel()), "upload_bytes_host_path": write_bytes,
           "jpeg_decode_included": False, "end_to_end_loader_measured": False}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
