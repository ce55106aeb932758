"""Deterministic mode on the GPU: the rewritten reduction sites give torch.equal results over repeated launches and still match
an fp64 reference; whole train steps at bench shapes give the same bits in two fresh processes."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def det():
    from gan_image_captioning_amd import engine
    before = engine.deterministic()
    engine.set_deterministic(True)
    yield
    engine.set_deterministic(before)


def _repeat(fn, n=5):
    outs = [fn() for _ in range(n)]
    torch.cuda.synchronize()
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    return outs[0]


@pytest.mark.parametrize("case", ["equal_ids", "random_ids"])
def test_embedding_bwd_is_bitwise_repeatable(det, case):
    from gan_image_captioning_amd import _lib as L
    from gan_image_captioning_amd.engine import ptr, stream_ptr
    torch.manual_seed(0)
    V, E = 10000, 512
    n = 64 if case == "equal_ids" else 1280
    ids = torch.full((n,), 7, dtype=torch.int64, device="cuda") if case == "equal_ids" else torch.randint(0, V, (n,), device="cuda")
    g = torch.randn(n, E, device="cuda")

    def run():
        dw = torch.empty(V, E, device="cuda")
        L.check(L.load().gic_embedding_bwd(ptr(g), ptr(ids), ptr(dw), n, V, E, 1, stream_ptr()), "gic_embedding_bwd")
        return dw
    dw = _repeat(run)
    ref = torch.zeros(V, E, dtype=torch.float64).index_add_(0, ids.cpu(), g.double().cpu())
    assert torch.allclose(dw.double().cpu(), ref, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_colsum_is_bitwise_repeatable(det, dtype, accumulate):
    from gan_image_captioning_amd import _lib as L
    from gan_image_captioning_amd.engine import ptr, stream_ptr
    torch.manual_seed(1)
    rows, cols = 8192, 900
    tdt, gdt = (torch.float32, L.F32) if dtype == "f32" else (torch.bfloat16, L.BF16)
    A = torch.randn(rows, cols, device="cuda").to(tdt)
    base = torch.randn(cols, device="cuda")

    def run():
        out = base.clone()
        L.check(L.load().gic_colsum(ptr(A), gdt, cols, rows, cols, ptr(out), accumulate, stream_ptr()), "gic_colsum")
        return out
    out = _repeat(run)
    ref = A.double().sum(0).cpu() + (base.double().cpu() if accumulate else 0)
    assert torch.allclose(out.double().cpu(), ref, rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("shape", [(900, 900, 8192), (64, 2048, 1024), (512, 512, 1280)])
def test_split_k_gemm_is_bitwise_repeatable(det, shape):
    from gan_image_captioning_amd import engine
    torch.manual_seed(2)
    M, N, K = shape
    A = torch.randn(K, M, device="cuda").bfloat16()          # weight-gradient form: both operands row-major over K
    B = torch.randn(K, N, device="cuda").bfloat16()

    def run():
        C = torch.empty(M, N, device="cuda")
        engine.gemm(A, B, C, M, N, K, M, N, N, a_kc=False, b_kc=False)
        return C
    C = _repeat(run)
    ref = A.double().t() @ B.double()
    assert torch.allclose(C.double(), ref, rtol=1e-3, atol=5e-2)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("rows,C", [(802816, 64), (200704, 256), (3136, 2048)])
def test_bn_stats_is_bitwise_repeatable(det, dtype, rows, C):
    import ctypes
    from gan_image_captioning_amd import _lib as L
    from gan_image_captioning_amd.engine import ptr, stream_ptr
    torch.manual_seed(3)
    tdt, gdt = (torch.float32, L.F32) if dtype == "f32" else (torch.bfloat16, L.BF16)
    y = (torch.randn(rows, C, device="cuda") + 0.5).to(tdt)
    need = ctypes.c_int64()
    L.check(L.load().gic_bn_stats_slab_floats(rows, C, ctypes.byref(need)), "gic_bn_stats_slab_floats")
    slab = torch.empty(need.value, device="cuda")

    def run():
        st = torch.empty(2 * C, device="cuda")
        L.check(L.load().gic_bn_stats(ptr(y), gdt, rows, C, ptr(slab), ptr(st), stream_ptr()), "gic_bn_stats")
        return st
    st = _repeat(run)
    yd = y.double()
    ref = torch.cat([yd.sum(0), (yd * yd).sum(0)]).cpu()
    assert torch.allclose(st.double().cpu(), ref, rtol=1e-4, atol=1e-2)


def _bench_digest(tmp, tag, dtype):
    out = os.path.join(tmp, tag)
    env = dict(os.environ, GIC_DETERMINISTIC="1")
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "0", "--dtype", dtype, "--no-cpu-baseline",
           "--no-roofline", "--dump-outputs", out]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    return {n: np.load(os.path.join(out, n + ".npy")) for n in ("losses", "gen_params", "disc_params")}


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_bench_steps_are_bitwise_equal_in_fresh_processes(tmp_path, dtype):
    # the flagship step (cfg2: B=64, L=20, V=10000, E=H=512, R50@224 trunk, fused driver, device-drawn noise): three optimizer
    # steps in two fresh processes, one after the other
    a = _bench_digest(str(tmp_path), "a", dtype)
    b = _bench_digest(str(tmp_path), "b", dtype)
    for n in a:
        assert np.isfinite(a[n]).all(), n
        assert a[n].tobytes() == b[n].tobytes(), f"{n} differs between two deterministic runs"
