"""Which kernel every dense product and trunk convolution takes, pinned without a GPU.

Route-only mode (gicap.h gic_debug_route_only) makes the library's GEMM / convolution entry points validate and select, and then
return without touching the GPU: the pointers below are fake, 16-byte aligned and never dereferenced.

Every expected string is one row of a rocprofv3 kernel trace of the commit BEFORE selection and launch were separated (eager launches,
MI355X): the kernel instantiation with its template arguments in their order, the grid in workgroups (the trace's Grid_Size / Workgroup_Size;
for the 4-wave kernel tiles x splits) and the workgroup size.  The traced programs: `bench.py` cfg2 (its ResNet-50 trunk at 224 x 224, batch
64, and the train step's products, whose shapes GIC_GEMM_LOG=1 listed), the trunk alone at 224 / 64 with GIC_NO_CONV_B2B=1 (the rows marked
"b2b off": the only runs in which gic_conv1x1_res_in and conv3 through gic_conv2d_bn_in appear at that shape) and the trunk alone at 200 x 200,
batch 3.  conv_b2b's grid is min(row tiles, workgroups per CU x CUs), resolved at launch: the traces show it on 256 CUs.  The trace does not
report dynamic LDS: the expected `lds=` figure of a trunk row was recorded in route-only mode from the last commit whose select_* functions
spelled the byte count out by hand (0 for tile8 and the 4-wave kernel, which size their LDS statically).  select_* now takes it from the
layout the kernel addresses, so a figure that moves here is a kernel whose LDS image changed."""
import pytest

from gan_image_captioning_amd import _lib as L
from gan_image_captioning_amd import engine

P = 0x7F0000010000          # a fake, aligned, non-null device pointer
BF16, F32 = L.BF16, L.F32
UNSUPPORTED = L.ERR_UNSUPPORTED
INVALID_ARG = -1            # gic_status GIC_STATUS_INVALID_ARG


def conv2d(N, H, cin, cout, k, stride, pad, W=None, kw=None, dtype=BF16):
    return ("gic_conv2d", (P, P, P, P, 8, dtype, N, H, W or H, cin, cout, k, kw or k, stride, pad, None))


def conv2d_bn_in(N, H, cin, cout, k, stride, pad):
    return ("gic_conv2d_bn_in", (P, P, 8, P, P, float(N * H * H), P, P, P, 8, BF16, N, H, H, cin, cout, k, k, stride, pad, None))


def conv3_stats(rows, cin, cout):
    return ("gic_conv1x1_bn_in_stats", (P, P, 8, P, P, float(rows), P, P, 8, BF16, rows, cin, cout, None))


def res_in(N, H, cin, cout, projection):
    rs = P if projection else None
    return ("gic_conv1x1_res_in", (P, P, 8, P, P, P, rs, 8, rs, rs, float(N * H * H), P, P, P, P, 8, BF16, N, H, H, cin, cout, None))


def b2b(rows, c2, c1n, projection):
    rs = P if projection else None
    return ("gic_conv_b2b", (P, P, 8, P, P, P, P, 8, P, P, P, rs, 8, rs, rs, float(rows), P, P, P, P, 8, BF16, rows, c2, c1n, None))


def route(call):
    name, args = call
    with engine.route_only() as r:
        status = getattr(L.load(), name)(*args)
        line = r.last()
    return status, line


def kernel_and_grid(line):
    return line.split(" lds=")[0]


def lds_of(line):
    return int(line.split(" lds=")[1].split()[0])


R64 = 64 * 56 * 56           # rows of the 56 x 56 maps at batch 64: 200704; 28 x 28: 50176; 14 x 14: 12544; 7 x 7: 3136

# ResNet-50 trunk, training, bf16, 224 x 224, batch 64: every distinct convolution through the entry point the plan uses for it
TRUNK_224 = [
    ("stem", conv2d(64, 230, 4, 64, 7, 2, 0, kw=8), "conv_stem grid=256 block=512", 99328),
    ("2.0.conv1", conv2d(64, 56, 64, 64, 1, 1, 0), "conv1x1_stream<64,1,false,false> grid=256 block=512", 112640),
    ("2.x.conv2", conv2d_bn_in(64, 56, 64, 64, 3, 1, 1), "conv3x3_patch<64,6,false,true> grid=1600 block=512", 74240),
    ("2.x.conv3 stats", conv3_stats(R64, 64, 256), "conv1x1_stream<256,1,true,true> grid=256 block=512", 107008),
    ("2.0.downsample", conv2d(64, 56, 64, 256, 1, 1, 0), "conv1x1_stream<128,1,false,false> grid=256 block=512", 155648),
    ("2.0 -> 2.1.conv1", b2b(R64, 64, 64, True), "conv_b2b<64,64,false> grid=min(1568,2*cus) block=512", 70144),           # trace: 512
    ("2.1 -> 2.2.conv1", b2b(R64, 64, 64, False), "conv_b2b<64,64,true> grid=min(1568,2*cus) block=512", 70144),          # trace: 512
    ("2.2 -> 3.0.conv1", b2b(R64, 64, 128, False), "conv_b2b<64,128,true> grid=min(1568,1*cus) block=512", 102912),        # trace: 256
    ("3.0.conv2 (stride 2)", conv2d(64, 56, 128, 128, 3, 2, 1), "tile8<bf16,128,2,true,2,false,false,1024> grid=392 block=512", 0),
    ("3.x.conv3 stats", conv3_stats(R64 // 4, 128, 512), "conv1x1_stream<256,2,true,true> grid=256 block=512", 140288),
    ("3.0.downsample", conv2d(64, 56, 256, 512, 1, 2, 0), "tile8<bf16,128,2,true,1,false,false,1024> grid=1568 block=512", 0),
    ("3.0 -> 3.1.conv1", b2b(R64 // 4, 128, 128, True), "conv_b2b<128,128,false> grid=min(392,1*cus) block=512", 107520),   # trace: 256
    ("3.x.conv2", conv2d_bn_in(64, 28, 128, 128, 3, 1, 1), "conv3x3_patch<128,5,true,true> grid=392 block=512", 132096),
    ("3.1 -> 3.2.conv1", b2b(R64 // 4, 128, 128, False), "conv_b2b<128,128,true> grid=min(392,1*cus) block=512", 107520),   # trace: 256
    ("3.3 -> 4.0.conv1", b2b(R64 // 4, 128, 256, False), "conv_b2b<128,256,true> grid=min(392,1*cus) block=512", 156672),   # trace: 256
    ("4.0.conv2 (stride 2)", conv2d(64, 28, 256, 256, 3, 2, 1), "tile8<bf16,128,2,true,4,false,false,1024> grid=196 block=512", 0),
    ("4.x.conv3", conv2d_bn_in(64, 14, 256, 1024, 1, 1, 0), "conv1x1_pix<256,3,true> grid=196 block=512", 135168),
    ("4.0.downsample", conv2d(64, 28, 512, 1024, 1, 2, 0), "tile8<bf16,128,2,true,2,false,false,1024> grid=784 block=512", 0),
    ("4.x.conv1", conv2d(64, 14, 1024, 256, 1, 1, 0), "tile8<bf16,128,2,true,4,false,false,1024> grid=196 block=512", 0),
    ("4.x.conv2", conv2d_bn_in(64, 14, 256, 256, 3, 1, 1), "conv3x3_patch<128,4,true,true> grid=196 block=512", 116736),
    ("5.0.conv1", conv2d(64, 14, 1024, 512, 1, 1, 0), "tile8<bf16,128,2,true,2,false,false,1024> grid=392 block=512", 0),
    ("5.0.conv2 (stride 2)", conv2d(64, 14, 512, 512, 3, 2, 1), "tile8<bf16,64,2,true,4,false,false,1024> grid=200 block=512", 0),
    ("5.x.conv3", conv2d_bn_in(64, 7, 512, 2048, 1, 1, 0), "conv1x1_pix<512,2,false> grid=200 block=512", 135168),
    ("5.0.downsample", conv2d(64, 14, 1024, 2048, 1, 2, 0), "tile8<bf16,128,2,true,2,false,false,1024> grid=400 block=512", 0),
    ("5.x.conv1", conv2d(64, 7, 2048, 512, 1, 1, 0), "tile8<bf16,64,2,true,4,false,false,1024> grid=200 block=512", 0),
    ("5.x.conv2", conv2d_bn_in(64, 7, 512, 512, 3, 1, 1), "conv3x3_patch<64,4,true,true> grid=200 block=512", 94208),
    # b2b off: the block output formed on load by the next conv1, conv3 with bn2 on load
    ("b2b off 2.x.conv3", conv2d_bn_in(64, 56, 64, 256, 1, 1, 0), "conv1x1_stream<128,1,true,false> grid=256 block=512", 156160),
    ("b2b off 2.1.conv1", res_in(64, 56, 256, 64, True), "tile8<bf16,64,2,true,1,true,true,512> grid=1568 block=512", 0),
    ("b2b off 2.2.conv1", res_in(64, 56, 256, 64, False), "tile8<bf16,64,2,true,1,true,true,512> grid=1568 block=512", 0),
    ("b2b off 3.0.conv1", res_in(64, 56, 256, 128, False), "tile8<bf16,128,2,true,1,true,true,512> grid=1568 block=512", 0),
    ("b2b off 3.x.conv3", conv2d_bn_in(64, 28, 128, 512, 1, 1, 0), "conv1x1_stream<128,2,true,false> grid=256 block=512", 138240),
    ("b2b off 3.x.conv1", res_in(64, 28, 512, 128, False), "tile8<bf16,128,2,true,1,true,true,512> grid=392 block=512", 0),
]

# the same trunk at 200 x 200, batch 3 (maps of 50, 25, 13 and 7 pixels: 7500, 1875, 507 and 147 rows, none a multiple of 128)
TRUNK_200 = [
    ("stem", conv2d(3, 206, 4, 64, 7, 2, 0, kw=8), "conv_stem grid=150 block=512", 99328),
    ("2.0.conv1", conv2d(3, 50, 64, 64, 1, 1, 0), "tile8<bf16,64,2,true,4,false,false,1024> grid=59 block=512", 0),
    ("2.x.conv2", conv2d_bn_in(3, 50, 64, 64, 3, 1, 1), "conv3x3_patch<64,6,false,true> grid=60 block=512", 74240),
    ("2.x.conv3", conv2d_bn_in(3, 50, 64, 256, 1, 1, 0), "tile8<bf16,64,2,true,4,true,false,1024> grid=236 block=512", 0),
    ("2.0.downsample", conv2d(3, 50, 64, 256, 1, 1, 0), "tile8<bf16,64,2,true,4,false,false,1024> grid=236 block=512", 0),
    ("2.x.conv1", conv2d(3, 50, 256, 64, 1, 1, 0), "tile8<bf16,64,2,true,4,false,false,1024> grid=59 block=512", 0),
    ("3.0.conv1", conv2d(3, 50, 256, 128, 1, 1, 0), "tile8<bf16,64,2,true,4,false,false,1024> grid=118 block=512", 0),
    ("3.0.conv2 (stride 2)", conv2d(3, 50, 128, 128, 3, 2, 1), "tile8<bf16,64,2,true,4,false,false,1024> grid=30 block=512", 0),
    ("3.x.conv3", conv2d_bn_in(3, 25, 128, 512, 1, 1, 0), "tile8<bf16,64,2,true,4,true,false,1024> grid=120 block=512", 0),
    ("3.0.downsample", conv2d(3, 50, 256, 512, 1, 2, 0), "tile8<bf16,64,2,true,4,false,false,1024> grid=120 block=512", 0),
    ("3.x.conv1", conv2d(3, 25, 512, 128, 1, 1, 0), "tile8<bf16,64,2,true,4,false,false,1024> grid=30 block=512", 0),
    ("3.x.conv2", conv2d_bn_in(3, 25, 128, 128, 3, 1, 1), "conv3x3_patch<64,4,true,true> grid=30 block=512", 91136),
    ("4.0.conv1", conv2d(3, 25, 512, 256, 1, 1, 0), "tile8<bf16,64,2,true,4,false,false,1024> grid=60 block=512", 0),
    ("4.0.conv2 (stride 2)", conv2d(3, 25, 256, 256, 3, 2, 1), "tile8<bf16,64,2,true,4,false,false,1024> grid=16 block=512", 0),
    ("4.x.conv3", conv2d_bn_in(3, 13, 256, 1024, 1, 1, 0), "conv1x1_pix<256,3,true> grid=64 block=512", 135168),
    ("4.0.downsample", conv2d(3, 25, 512, 1024, 1, 2, 0), "tile8<bf16,64,2,true,4,false,false,1024> grid=64 block=512", 0),
    ("4.x.conv1", conv2d(3, 13, 1024, 256, 1, 1, 0), "tile8<bf16,64,2,true,4,false,false,1024> grid=16 block=512", 0),
    ("4.x.conv2", conv2d_bn_in(3, 13, 256, 256, 3, 1, 1), "conv3x3_patch<64,4,true,true> grid=16 block=512", 92160),
    ("5.0.conv1", conv2d(3, 13, 1024, 512, 1, 1, 0), "tile8<bf16,64,2,true,4,false,false,1024> grid=32 block=512", 0),
    ("5.0.conv2 (stride 2)", conv2d(3, 13, 512, 512, 3, 2, 1), "tile8<bf16,64,2,true,4,false,false,1024> grid=16 block=512", 0),
    ("5.x.conv3", conv2d_bn_in(3, 7, 512, 2048, 1, 1, 0), "conv1x1_pix<512,2,false> grid=64 block=512", 135168),
    ("5.0.downsample", conv2d(3, 13, 1024, 2048, 1, 2, 0), "tile8<bf16,64,2,true,4,false,false,1024> grid=64 block=512", 0),
    ("5.x.conv1", conv2d(3, 7, 2048, 512, 1, 1, 0), "tile8<bf16,64,2,true,4,false,false,1024> grid=16 block=512", 0),
    ("5.x.conv2", conv2d_bn_in(3, 7, 512, 512, 3, 1, 1), "conv3x3_patch<64,4,true,true> grid=16 block=512", 94208),
]


@pytest.mark.parametrize("name,call,expected,lds", TRUNK_224, ids=[c[0] for c in TRUNK_224])
def test_trunk_routes_at_224_batch_64(name, call, expected, lds):
    status, line = route(call)
    assert status == 0, line
    assert kernel_and_grid(line) == expected
    assert lds_of(line) == lds


@pytest.mark.parametrize("name,call,expected,lds", TRUNK_200, ids=[c[0] for c in TRUNK_200])
def test_trunk_routes_at_200_batch_3(name, call, expected, lds):
    status, line = route(call)
    assert status == 0, line
    assert kernel_and_grid(line) == expected
    assert lds_of(line) == lds


def test_rows_off_the_128_grid_decline_the_fused_pair():
    """200 x 200, batch 3: conv_b2b and its query decline every boundary (the plan then puts the BatchNorm on load: the tile8 rows with
    ABN above), and a 3x3 / stride 2 convolution has no BatchNorm on load (the plan runs gic_bn_act + gic_conv2d)."""
    lib = L.load()
    for rows, c2, c1n in ((7500, 64, 64), (7500, 64, 128), (1875, 128, 128), (1875, 128, 256)):
        assert lib.gic_conv_b2b_supported(BF16, rows, c2, c1n) == 0
        assert route(b2b(rows, c2, c1n, False)) == (UNSUPPORTED, "unsupported")
    assert lib.gic_conv_b2b_supported(F32, R64, 64, 64) == 0
    assert lib.gic_conv_b2b_supported(BF16, R64, 256, 256) == 0
    assert route(conv2d_bn_in(3, 50, 128, 128, 3, 2, 1)) == (UNSUPPORTED, "unsupported")
    assert route(conv3_stats(7500, 256, 1024)) == (UNSUPPORTED, "unsupported")       # the statistics-only pass exists for K = 64 | 128 only


def gemm(M, N, K, a_kc, b_kc, in_dt, out_dt, acc):
    up = lambda v: (v + 7) // 8 * 8                     # leading dimensions padded to whole 16-byte chunks, as the callers allocate them
    return ("gic_gemm", (P, P, P, M, N, K, up(K if a_kc else M), up(K if b_kc else N), up(N), a_kc, b_kc, in_dt, out_dt, None, acc, 1.0, None))


# every distinct plain product of one cfg2 train step: (M, N, K, a_kc, b_kc, in, out, accumulate) as GIC_GEMM_LOG=1 printed them
CFG2_PRODUCTS = [
    ((64, 512, 2048, 1, 1, BF16, F32, 0), "gemm<bf16,f32,true,true,64,64,true,0,false,false> grid=8x16 block=256", 16),
    ((64, 10000, 1280, 0, 0, BF16, F32, 1), "gemm<bf16,f32,false,false,64,64,true,0,false,false> grid=157x3 block=256", 3),
    ((100, 900, 8192, 0, 0, BF16, F32, 1), "gemm<bf16,f32,false,false,64,64,true,0,false,false> grid=30x16 block=256", 16),
    ((512, 2048, 64, 0, 0, BF16, F32, 0), "gemm<bf16,f32,false,false,64,64,true,0,false,false> grid=256x1 block=256", 1),
    ((900, 900, 8192, 0, 0, BF16, F32, 1), "gemm<bf16,f32,false,false,64,64,true,0,false,false> grid=225x3 block=256", 3),
    ((1280, 64, 10000, 1, 1, BF16, F32, 0), "gemm<bf16,f32,true,true,64,64,true,0,false,true> grid=20x12 block=256", 12),
    ((1280, 512, 2048, 1, 1, BF16, F32, 0), "gemm<bf16,f32,true,true,64,64,true,0,false,true> grid=160x3 block=256", 3),
    ((1280, 512, 10000, 1, 0, BF16, F32, 0), "gemm<bf16,f32,true,false,64,64,true,0,false,false> grid=160x3 block=256", 3),
    ((1280, 10000, 64, 1, 0, BF16, BF16, 0), "gemm<bf16,bf16,true,false,128,128,true,0,false,false> grid=790x1 block=256", 1),
    ((2048, 512, 1280, 0, 0, BF16, F32, 0), "gemm<bf16,f32,false,false,64,64,true,0,false,false> grid=256x1 block=256", 1),
    ((4096, 100, 960, 1, 1, BF16, F32, 0), "gemm<bf16,f32,true,true,64,64,true,0,false,true> grid=128x1 block=256", 1),
    ((4096, 960, 104, 1, 0, BF16, F32, 0), "gemm<bf16,f32,true,false,128,128,true,0,false,false> grid=256x1 block=256", 1),
    ((4096, 960, 960, 1, 1, BF16, F32, 1), "tile8<f32,128,0,false,4,false,false,1024> grid=256 block=512", None),
    ((8192, 960, 104, 1, 0, BF16, F32, 0), "gemm<bf16,f32,true,false,128,128,true,0,false,false> grid=512x1 block=256", 1),
    ((8192, 960, 960, 1, 1, BF16, F32, 1), "tile8<f32,128,0,false,2,false,false,1024> grid=512 block=512", None),
    ((10000, 512, 1280, 0, 0, BF16, F32, 0), "gemm<bf16,f32,false,false,128,128,true,0,false,false> grid=316x1 block=256", 1),
]


def splits_of(line):
    return int(line.split(" splits=")[1].split()[0])


@pytest.mark.parametrize("shape,expected,splits", CFG2_PRODUCTS, ids=["x".join(map(str, c[0][:3])) for c in CFG2_PRODUCTS])
def test_cfg2_product_routes(shape, expected, splits):
    status, line = route(gemm(*shape))
    assert status == 0, line
    assert kernel_and_grid(line) == expected
    if splits is not None:
        assert splits_of(line) == splits
        # deterministic mode: two splits onto a zeroed C at the most, none onto a C that is accumulated into
        engine.set_deterministic(True)
        try:
            status, line = route(gemm(*shape))
        finally:
            engine.set_deterministic(False)
        assert status == 0 and line.startswith("gemm<")
        assert splits_of(line) == (1 if shape[7] or splits == 1 else 2)


def disc_fwd(rows, train=1, dtype=BF16, **state):
    """gic_disc_fwd over rows = B * R feature rows of cfg2's discriminator (F = 900 filters in Fp = 960 columns, R = 64): in route-only mode
    the call selects its highway product (M = rows, N = F, K = Fp: the one caller of the highway epilogue) and launches nothing.  `state`
    replaces buffers of the saved state (hpre, keep, ydrop ...); every other pointer is P."""
    d, prm, sh, st = L.DiscDims(), L.DiscParams(), L.DiscShadow(), L.DiscState()
    d.B, d.L, d.V, d.De, d.R, d.nconv = rows // 64, 20, 10000, 64, 64, 1
    d.fsize[0], d.nfilt[0] = 2, 900                     # (the filter bank does not enter the highway product: one bank of all F filters)
    d.F, d.Fp, d.dtype, d.drop_p = 900, 960, dtype, 0.2
    for s in (prm, sh, st):
        for name, ctype in s._fields_:
            setattr(s, name, P if ctype is L.c_void_p else ctype(P))
    for name, ptr in state.items():
        setattr(st, name, ptr)
    return ("gic_disc_fwd", (d, prm, sh, st, None, 0, P, train, None, 1, P, None, 0, None))


# the discriminator passes of one cfg2 train step: B = 64 captions, and the real + fake pair of 128
@pytest.mark.parametrize("rows,expected", [(4096, "tile8<bf16,128,1,false,4,false,false,1024> grid=256 block=512"),
                                           (8192, "tile8<bf16,128,1,false,2,false,false,1024> grid=512 block=512")])
def test_cfg2_highway_routes(rows, expected):
    for train in (1, 0):
        status, line = route(disc_fwd(rows, train))
        assert status == 0, line
        assert kernel_and_grid(line) == expected
    # a forward that no backward follows saves no pre-activation: the same kernel, which skips the store
    status, line = route(disc_fwd(rows, 0, hpre=None, argmax=None))
    assert status == 0 and kernel_and_grid(line) == expected, line


@pytest.mark.parametrize("state", [{"hpre": P + 8}, {"ydrop": P + 8}, {"keep": P + 4}], ids=lambda s: next(iter(s)))
def test_highway_off_its_row_padded_form_takes_the_4_wave_kernel(state):
    """tile8's highway epilogue owns 4-row x 8-column patches with 16-byte accesses to C / X / Hpre and 8-byte ones to the keep mask: a
    buffer that is not aligned for them sends the product to gemm_kernel, whose highway epilogue is element-wise."""
    status, line = route(disc_fwd(4096, 1, **state))
    assert status == 0, line
    assert kernel_and_grid(line) == "gemm<bf16,bf16,true,true,128,128,true,1,false,true> grid=256x1 block=256"     # (K = 15 tiles over 256 blocks: the LDS-DMA ring)
    status, line = route(disc_fwd(4096, 1))
    assert status == 0 and line.startswith("tile8<bf16,128,1,"), line


# ---------------------------------------------------------------------------------------------------------------- the discriminator's own kernels
def disc_dims(rows, dtype=BF16, L_=20, fs=(3, 4, 5), nf=(300, 300, 300), R=64, fp_align=64):
    """cfg2's discriminator as bench.py builds it (default_args: disc_embed_dim = disc_num_rep = 64, filter sizes 3 / 4 / 5 with 300 filters
    each, captions of 20 tokens, 10000 words; Fp = F rounded up to 64 columns) over rows = B * 64 feature rows."""
    d = L.DiscDims()
    d.B, d.L, d.V, d.De, d.R, d.nconv = rows // R, L_, 10000, R, R, len(fs)
    for k, (f, n) in enumerate(zip(fs, nf)):
        d.fsize[k], d.nfilt[k] = f, n
    d.F = sum(nf)
    d.Fp, d.dtype, d.drop_p = (d.F + fp_align - 1) // fp_align * fp_align, dtype, 0.2
    return d


def disc_plan(d, flags):
    import ctypes
    out = ctypes.create_string_buffer(2048)
    status = L.load().gic_debug_disc_plan(ctypes.byref(d), flags, out, len(out))
    return status, out.value.decode().splitlines()


# (kernel, workgroups at 4096 rows, at 8192 rows, workgroup size, dynamic LDS bytes); the LDS figure is the parent's launch-site expression
# at L = 20, s = 1, R = 64, worked out by hand:
CFG2_DISC_FWD_TRAIN = ("disc_conv_pool_fwd_mfma_kernel<bf16>", "256", "512", 512, 0)             # `0`: the kernel's LDS is static
CFG2_DISC_FWD_ONLY = ("disc_conv_pool_fwd_bf16_kernel<bf16>", "128", "256", 512, 13952)          # 32 * L * 16 + 32 * (L + 9) * 4 = 10240 + 3712
CFG2_DISC_BWD = [
    ("disc_out_bwd_kernel<bf16>", "256", "256", 256, 0),                                          # `0`
    ("disc_out_fold_kernel", "1", "1", 128, 0),                                                   # `0`; deterministic mode only
    ("disc_highway_bwd_vec_kernel<bf16>", "1920", "2048", 256, 0),                                # `0`
    ("disc_conv_pool_bwd_w_lds_kernel<bf16,8>", "15x64", "15x64", 256, 7424),                     # R * ((L + 8) | 1) * sizeof(float) = 64 * 29 * 4
    ("disc_wgrad_fold_kernel", "32", "32", 256, 0),                                               # `0`; deterministic mode only
    ("disc_conv_pool_bwd_x_small_kernel<bf16,32,8>", "1024", "2048", 256, 20480),                 # n_out * 256 * sizeof(float) = 20 * 256 * 4
]
FOLDS = ("disc_out_fold_kernel", "disc_wgrad_fold_kernel")


@pytest.mark.parametrize("rows", [4096, 8192])
def test_cfg2_discriminator_plan(rows):
    """The kernels gic_disc_fwd / gic_disc_bwd launch of their own for the bench.py cfg2 discriminator, per mode, as gic_debug_disc_plan
    (the library's select_disc_fwd / select_disc_bwd) prints them.  Kernel names with their template arguments, grids and workgroup
    sizes are rows of ONE rocprofv3 --kernel-trace run (no counters, MI355X) of the commit before selection and launch were separated in
    csrc/disc.hip: an eager DiscEngine.fwd + .bwd (token ids, parameter gradients) per mode -- train, forward-only (eval, no saved state),
    deterministic -- at B = 64 and 128; the rows are kept in profiles/disc_plan_trace.txt (Grid_Size / Workgroup_Size = workgroups).
    The trace does not report dynamic LDS: each figure is that commit's launch-site expression, quoted beside its value above.
    Outside the deterministic mode nothing is folded; in it both partial sums are (dydrop's 4096 * 960 floats hold 256 * 101 and
    64 * 900 * 9 of them), and rpb = 4 from 2048 rows on."""
    col = 1 if rows == 4096 else 2
    line = lambda r, extra="": f"{r[0]} grid={r[col]} block={r[3]} lds={r[4]}{extra}"
    bwd = lambda det: [line(r, {0: f" blocks=256 part={det}", 3: f" rows_y=64 part={det}", 5: " rpb=4"}.get(i, ""))
                       for i, r in enumerate(CFG2_DISC_BWD) if det or r[0] not in FOLDS]
    d = disc_dims(rows)
    assert disc_plan(d, L.DISC_PLAN_GRADS | L.DISC_PLAN_TRAIN) == (0, [line(CFG2_DISC_FWD_TRAIN)] + bwd(0))
    status, lines = disc_plan(d, L.DISC_PLAN_NO_ARGMAX)
    assert status == 0 and lines[0] == line(CFG2_DISC_FWD_ONLY)
    eng = engine.DiscEngine(10000, 64, 64, [3, 4, 5], [300, 300, 300], BF16)                  # the Python wrapper: the same lines
    assert eng.plan(rows // 64, 20) == [line(CFG2_DISC_FWD_TRAIN)] + bwd(0)
    assert eng.plan(rows // 64, 20, want_param_grads=False, train=False, keeps_argmax=False)[0] == line(CFG2_DISC_FWD_ONLY)
    engine.set_deterministic(True)
    try:
        assert disc_plan(d, L.DISC_PLAN_GRADS | L.DISC_PLAN_TRAIN) == (0, [line(CFG2_DISC_FWD_TRAIN)] + bwd(1))
        # the generator's path through D (no parameter gradients): nothing to fold in either mode, no weight gradient
        assert disc_plan(d, L.DISC_PLAN_TRAIN)[1] == [line(CFG2_DISC_FWD_TRAIN)] + [l for l in bwd(0) if "bwd_w" not in l]
    finally:
        engine.set_deterministic(False)


def fake(struct):
    for name, ctype in struct._fields_:
        setattr(struct, name, P if ctype is L.c_void_p else ctype(*[P] * ctype._length_))
    return struct


def disc_bwd_call(d, grads=True):
    import ctypes
    g = ctypes.byref(fake(L.DiscGrads())) if grads else None
    return ("gic_disc_bwd", (d, fake(L.DiscParams()), fake(L.DiscShadow()), fake(L.DiscState()), fake(L.DiscBwdWs()), None, 0, P, 1, P, g, 0, None, 0, None))


def test_conv_weights_beyond_the_lds_staging_are_refused():
    """The general input-gradient kernel stages every conv weight in LDS beside 3 * Fp + NG * n_out floats (256 at L * s = 32): 1168
    filters of 32 taps (s = 1, L = 32: f * s <= 32, f <= L and nconv <= 8 hold, make_ctx accepts the bank; Fp = F) come to 3504 + 256 +
    37376 = 41136 floats, past the 160 KB = 40960 floats a workgroup can have; 1160 filters to 40856.  The query and the backward
    (route-only mode: fake pointers) refuse the first with select_disc_bwd's message."""
    lib = L.load()
    d = disc_dims(64, L_=32, fs=(32,), nf=(1168,), fp_align=8)
    assert lib.gic_disc_state_bytes(d, (L.C.c_uint64 * 7)()) == 0                      # make_ctx's own limits do not refuse it
    assert disc_plan(d, L.DISC_PLAN_GRADS | L.DISC_PLAN_TRAIN) == (INVALID_ARG, [])
    assert lib.gic_last_error() == b"disc_bwd: conv weights (37376 floats) do not fit the LDS staging"
    assert lib.gic_disc_state_bytes(None, None) == INVALID_ARG                         # (another message in between)
    assert route(disc_bwd_call(d))[0] == INVALID_ARG
    assert lib.gic_last_error() == b"disc_bwd: conv weights (37376 floats) do not fit the LDS staging"
    ok = disc_dims(64, L_=32, fs=(32,), nf=(1160,), fp_align=8)
    assert disc_plan(ok, L.DISC_PLAN_GRADS)[1][-1] == "disc_conv_pool_bwd_x_kernel<bf16> grid=64 block=256 lds=163424"
    assert route(disc_bwd_call(ok))[0] == 0


def test_route_only_discriminator_backward_and_redrop_launch_nothing():
    """gic_disc_bwd, gic_disc_bwd_cond and gic_disc_fwd_redrop in route-only mode: validated, selected, status returned -- over fake
    pointers, on a machine that may have no GPU at all.  (They used to run their fills, column sums and own kernels over them.)"""
    lib = L.load()
    d = disc_dims(4096)
    with engine.route_only() as r:
        lib.gic_gemm(*gemm(64, 512, 2048, 1, 1, BF16, F32, 0)[1])
        line = r.last()
        for grads in (True, False):
            assert getattr(lib, "gic_disc_bwd")(*disc_bwd_call(d, grads)[1]) == 0, lib.gic_last_error()
        assert lib.gic_disc_bwd_cond(*disc_bwd_call(d)[1][:-1], P, 0.03, P, None) == 0, lib.gic_last_error()
        assert lib.gic_disc_fwd_redrop(d, fake(L.DiscParams()), fake(L.DiscShadow()), fake(L.DiscState()), fake(L.DiscState()), 1, None, 1, P,
                                       None, 0, None) == 0, lib.gic_last_error()
        assert r.last() == line                                 # none of them selects a product of its own
        # ... and validation still comes first
        assert lib.gic_disc_bwd(d, fake(L.DiscParams()), fake(L.DiscShadow()), fake(L.DiscState()), fake(L.DiscBwdWs()), None, 0, None, 1, P, None, 0,
                                None, 0, None) == INVALID_ARG
        assert b"pass inp_soft, inp_ids" in lib.gic_last_error()


def test_fp32_highway_takes_the_4_wave_kernel():
    status, line = route(disc_fwd(4096, 1, dtype=F32))
    assert status == 0 and line.startswith("gemm<f32,f32,true,true,128,128,true,1,false,"), line


def test_fp32_takes_the_4_wave_kernel():
    status, line = route(gemm(4096, 960, 960, 1, 1, F32, F32, 0))          # a shape tile8 takes in bf16
    assert status == 0 and line.startswith("gemm<f32,f32,true,true,"), line
    assert splits_of(line) == 1                                            # the parity mode never splits K
    status, line = route(conv2d(64, 56, 64, 64, 1, 1, 0, dtype=F32))       # ... and one the streaming kernel takes
    assert status == 0 and line.startswith("gemm<f32,f32,true,true,"), line


def test_b2b_declines_what_its_byte_offsets_cannot_reach():
    """rows * 4 * C2 * 2 >= 2^31: the library's query declines, and so does the plan's _b2b_ok (which used to restate the shape table
    without this bound: the statistics-only pass then ran and gic_conv_b2b raised after it)."""
    from gan_image_captioning_amd.trunk import ResNetTrunk
    from gan_image_captioning_amd.encoder_engine import TrunkPlan
    lib = L.load()
    rows = (1 << 31) // (4 * 64 * 2)                  # 4194304, a multiple of 128
    assert lib.gic_conv_b2b_supported(BF16, rows - 128, 64, 64) == 1
    assert lib.gic_conv_b2b_supported(BF16, rows, 64, 64) == 0
    assert route(b2b(rows, 64, 64, False)) == (UNSUPPORTED, "unsupported")
    plan = TrunkPlan(ResNetTrunk("resnet50"), BF16)
    blk, nxt = plan.blocks[0], plan.blocks[1]
    assert plan._b2b_ok(blk, nxt, rows - 128, True)
    assert not plan._b2b_ok(blk, nxt, rows, True)


def test_route_only_is_cleared_on_exit():
    lib = L.load()
    empty = (P, P, P, 0, 8, 8, 8, 8, 8, 1, 1, BF16, F32, None, 0, 1.0, None)      # M = 0: GIC_OK with nothing to do, in either mode
    with pytest.raises(RuntimeError):
        with engine.route_only():
            getattr(lib, "gic_gemm")(*gemm(64, 512, 2048, 1, 1, BF16, F32, 0)[1])
            raise RuntimeError("boom")
    line = engine.route_only.last()
    assert line.startswith("gemm<")
    assert lib.gic_gemm(*empty) == 0
    assert engine.route_only.last() == line               # flag off: the call did not look at the route line
    with engine.route_only() as r:
        assert lib.gic_gemm(*empty) == 0
        assert r.last() == ""                             # flag on: an empty product selects nothing


# ---------------------------------------------------------------------------------------------------------------- the decoder passes
# gic_debug_decoder_plan / gic_debug_step_plan (csrc/decoder_step.h select_decoder_fwd / select_decoder_bwd / select_lstm_step /
# select_vocab_step) and the decoder entry points in route-only mode.  Kernel names, grids and workgroup sizes of the cfg2 rows are rows of
# ONE rocprofv3 --kernel-trace run (no counters, MI355X; tools/decoder_plan_trace.py) of the commit before selection and launch were
# separated in the decoder passes, kept in profiles/decoder_plan_trace.txt (Grid_Size / Workgroup_Size = workgroups).  The trace does not
# report dynamic LDS: each lds= figure is that commit's launch-site expression, restated below and worked out beside its value.
import ctypes
import os
import subprocess
import sys

from tests import decode_ws as W

DEV_SCALARS_REFUSAL = (b"decoder_sample_fwd: device-resident step scalars need the fused step kernels (state->part, B <= 512, V % 4 == 0, "
                       b"E, H % 8 == 0)")
PL = L      # (the module; `L` is a caption length in some signatures below)


def dsz(dt):
    return 4 if dt == F32 else 2


def up32(n):
    return (n + 31) // 32 * 32


# the parent commit's launch-site formulae (decoder_step.hip): the K chunk staged per pass and the dynamic LDS of the two step kernels
def lstm_chunk(dt, ldx):
    return min(up32(ldx), 2048 // dsz(dt))                                  # 2 KiB of a row


def lstm_lds(dt, ldx):
    return max(64 * (lstm_chunk(dt, ldx) * dsz(dt) + 16), 8 * 64 * 17 * 4)    # one staged tile | the reduction scratch (34816)


def vocab_chunk(dt, H):
    return min(up32(H), 1024 // dsz(dt))                                    # 1 KiB of a row


def vocab_lds(dt, H, beam=False):
    lds = max(2 * 64 * (vocab_chunk(dt, H) * dsz(dt) + 16), 8 * 2 * 64 * 16 + 4 * 4 * 64 * 4)     # two staged tiles | the epilogue scratch (20480)
    return max(lds, 64 * 65 * 4) if beam else lds                           # the beam forms' logits tile: 16640


def tname(dt):
    return "f32" if dt == F32 else "bf16"


def lstm_line(dt, B, H, ldx, variant=0):
    k = ("lstm_step_kernel", "lstm_step_pack_kernel", "lstm_step_beam_kernel")[variant]
    return f"{k}<{tname(dt)}> grid={-(-H // 4)}x{-(-B // 64)} block=512 lds={lstm_lds(dt, ldx)} KC={lstm_chunk(dt, ldx)}"


def vocab_line(dt, B, V, H, variant=0, K=0):
    k = ("vocab_step_kernel", "vocab_step_logits_kernel", "vocab_step_beam_kernel", "vocab_step_beam_ban_kernel", "vocab_step_beam_hop_kernel")[variant]
    targ = ("true" if dt == BF16 else "false") if variant == 0 else K
    args = tname(dt) if variant == 1 else f"{tname(dt)},{targ}"
    return f"{k}<{args}> grid={-(-V // 64)}x{-(-B // 64)} block=512 lds={vocab_lds(dt, H, variant >= 2)} KC={vocab_chunk(dt, H)}"


def step_plan(lstm, variant, dt, B, H, ldx_or_V, K=0):
    out = ctypes.create_string_buffer(256)
    assert PL.load().gic_debug_step_plan(lstm, variant, dt, B, H, ldx_or_V, K, out, len(out)) == 0
    return out.value.decode()


def decoder_plan(B, Lc, V, E, H, NL=1, dt=BF16, flags=0):
    out = ctypes.create_string_buffer(4096)
    status = PL.load().gic_debug_decoder_plan(ctypes.byref(PL.DecoderDims(B, Lc, V, E, H, NL, dt)), flags, out, len(out))
    return status, out.value.decode().splitlines()


def fwd_path(lines):
    return lines[0].split("path=")[1].split()[0]


def bwd_path(lines):
    return next(l for l in lines if l.startswith("backward ")).split("path=")[1]


TRAIN, PRETRAIN, DEVS, RESUMED, NO_PART, NO_WCAT_T, STATE_GRADS, LOGITS_4 = (
    PL.DECODER_PLAN_TRAIN, PL.DECODER_PLAN_PRETRAIN, PL.DECODER_PLAN_DEV_SCALARS, PL.DECODER_PLAN_RESUMED, PL.DECODER_PLAN_NO_PART,
    PL.DECODER_PLAN_NO_WCAT_T, PL.DECODER_PLAN_STATE_GRADS, PL.DECODER_PLAN_LOGITS_UNALIGNED)


def test_cfg2_decoder_plan():
    """bench.py's cfg2 decoder (B = 64, L = 20, V = 10000, E = H = 512, NL = 1, bf16): the train plan (phase 1 of the trace: roll-out and
    backward on the fused step kernels) and the ids-only plan.  Trace rows: lstm_step_kernel<bf16> 65536x1 / 512 = 128 workgroups, x20;
    vocab_step_kernel<bf16,true> 80384x1 / 512 = 157, x20; sample_finish_kernel<bf16> 327680 / 256 = 1280; softmax_bwd_vec_kernel<bf16,5>
    1280 blocks of 256; lstm_bwd_step_kernel<bf16,8> 16384x4 / 512 = 32x4, x20.  LDS: lstm_lds_bytes = 64 * (1024 * 2 + 16) = 132096 (ldx =
    1024 = the 2 KiB chunk); vocab_lds_bytes = 2 * 64 * (512 * 2 + 16) = 133120."""
    fwd = ["forward path=FUSED from=0",
           "lstm_step_kernel<bf16> grid=128x1 block=512 lds=132096 KC=1024 x20",
           "vocab_step_kernel<bf16,true> grid=157x1 block=512 lds=133120 KC=512 x20",
           "sample_finish_kernel<bf16> grid=1280 block=256 lds=0 x1"]
    status, lines = decoder_plan(64, 20, 10000, 512, 512, flags=TRAIN)
    assert status == 0 and lines[:4] == fwd
    assert lines[4:7] == ["backward path=FUSED", "softmax_bwd_vec_kernel<bf16,5> grid=1280 block=256 lds=0 x1",
                          "lstm_bwd_step_kernel<bf16,8> grid=32x4 block=512 lds=0 x20"]
    # d x_0 = dgates W_ih over all L * B rows, then the weight gradient as ONE product with both bias sums folded in (CFG2_PRODUCTS above
    # has the two shapes' plain routes)
    assert kernel_and_grid(lines[7]) == "gemm<bf16,f32,true,true,64,64,true,0,false,true> grid=160x3 block=256" and lines[7].endswith("M=1280 N=512 K=2048 x1")
    assert kernel_and_grid(lines[8]) == "gemm<bf16,f32,false,false,64,64,true,0,false,false> grid=512x1 block=256"
    assert lines[8].endswith("a_sum=2 n_split=512 M=2048 N=1024 K=1280 x1") and len(lines) == 9
    assert decoder_plan(64, 20, 10000, 512, 512, flags=0) == (0, fwd)             # ids only: the same roll-out, no backward
    assert lines[1].rsplit(" x", 1)[0] == lstm_line(BF16, 64, 512, 1024) and lines[2].rsplit(" x", 1)[0] == vocab_line(BF16, 64, 10000, 512)
    eng = engine.DecoderEngine(10000, 512, 512, 1, BF16)                          # the Python wrapper: the same lines
    assert eng.plan(64, 20) == lines and eng.plan(64, 20, train=False) == fwd
    # the f32 twin takes the <float, ...> instantiations: half the elements per chunk, the same bytes
    status, f32 = decoder_plan(64, 20, 10000, 512, 512, dt=F32, flags=TRAIN)
    assert status == 0 and f32[:7] == ["forward path=FUSED from=0",
                                       "lstm_step_kernel<f32> grid=128x1 block=512 lds=132096 KC=512 x20",
                                       "vocab_step_kernel<f32,false> grid=157x1 block=512 lds=133120 KC=256 x20",
                                       "sample_finish_kernel<f32> grid=1280 block=256 lds=0 x1", "backward path=FUSED",
                                       "softmax_bwd_kernel<f32> grid=1280 block=256 lds=0 x1",          # V = 10000 > 256 * 8 * 4: the scalar kernel
                                       "lstm_bwd_step_kernel<f32,4> grid=32x4 block=512 lds=0 x20"]
    assert f32[-1] == "colsum x1" and len(f32) == 11                               # no folded form in f32: two products and colsum


# the one predicate at the smallest shapes that flip it: (B, L, V, E, H, NL), flags -> the forward's path.  Base: 2, 3, 8, 8, 8, 1.
BASE = (2, 3, 8, 8, 8, 1)
EDGES = [
    ("base", BASE, 0, "FUSED"), ("V % 4", (2, 3, 10, 8, 8, 1), 0, "GENERIC"), ("V = 4", (2, 3, 4, 8, 8, 1), 0, "FUSED"),
    ("V = 3", (2, 3, 3, 8, 8, 1), 0, "GENERIC"), ("V = 6", (2, 3, 6, 8, 8, 1), 0, "GENERIC"), ("E % 8", (2, 3, 8, 12, 8, 1), 0, "GENERIC"),
    ("H % 8", (2, 3, 8, 8, 12, 1), 0, "GENERIC"), ("1024 tiles", (2, 3, 64 * 1024, 8, 8, 1), 0, "FUSED"),
    ("1025 tiles", (2, 3, 64 * 1024 + 4, 8, 8, 1), 0, "GENERIC"), ("512 rows", (512, 3, 8, 8, 8, 1), 0, "FUSED"),
    ("513 rows", (513, 3, 8, 8, 8, 1), 0, "GENERIC"), ("no part", BASE, NO_PART, "GENERIC"), ("resumed", BASE, RESUMED, "GENERIC"),
]


@pytest.mark.parametrize("name,shape,flags,path", EDGES, ids=[e[0] for e in EDGES])
def test_one_predicate_decides_every_decoder_path(name, shape, flags, path):
    """select_decoder_fwd's answer at every edge, and -- the assertion that the copies are one -- the same answer from
    gic_decoder_fused_rollout_rows, from decode.hip's d.fused (through the workspace queries: the gpre / logits regions are there or
    not) and from the teacher-forced decode's fused-logits choice (the route-only plan of gic_decoder_forward_ss).  Device-resident step
    scalars off the fused path are refused with the message recorded from the commit before the refactor."""
    lib = PL.load()
    B, Lc, V, E, H, NL = shape
    for dt in (BF16, F32):
        status, lines = decoder_plan(*shape, dt=dt, flags=flags | TRAIN)          # (train: `out` is there, no row keys)
        assert status == 0 and fwd_path(lines) == path, lines
        status, lines = decoder_plan(*shape, dt=dt, flags=flags | TRAIN | DEVS)
        if path == "FUSED":
            assert status == 0 and fwd_path(lines) == "FUSED"
        else:
            assert (status, lines) == (UNSUPPORTED, []) and lib.gic_last_error() == DEV_SCALARS_REFUSAL
        shapes_fused = path == "FUSED" or bool(flags)                             # part / resume_from are facts of a call, not of the shapes
        rows = ctypes.c_int32(-1)
        assert lib.gic_decoder_fused_rollout_rows(ctypes.byref(PL.DecoderDims(*shape, dt)), ctypes.byref(rows)) == 0
        assert (B <= rows.value) == shapes_fused and rows.value in (0, 512)
        if V <= 4096:                                                             # (the workspace queries take any V; keep the replica small)
            d, eng = W.Dims(B, Lc, V, E, H, NL), engine.DecoderEngine(V, E, H, NL, dt)
            for beam in (True, False):
                want, other = (W.decode_regions(d, 1, dt, beam, f)[1] for f in (shapes_fused, not shapes_fused))
                got = eng.beam_ws_bytes(B, Lc, 1) if beam else eng.sample_ws_bytes(B, Lc, 1)
                assert got == want and got != other
        status, line = route(forward_ss_call(shape, dt))
        assert status == 0, lib.gic_last_error()
        assert line.startswith("gemm<") and line.endswith(" ss_logits=fused") == shapes_fused, line      # (the logits product, or the gates')


def fake_decoder(NL=1, **state):
    prm, sh, st = fake(PL.DecoderParams()), fake(PL.DecoderShadow()), fake(PL.DecoderState())
    for name, ptr in state.items():
        setattr(st, name, ptr)
    return prm, sh, st


def forward_ss_call(shape, dt):
    B, Lc, V, E, H, NL = shape
    opts = PL.SchedSampleOpts(0.25, 0, None, None, 1, P, P)
    return ("gic_decoder_forward_ss", (PL.DecoderDims(B, Lc + 1, V, E, H, NL, dt), *fake_decoder(NL), P, P, P, Lc, opts, P, P, P, P, None))


def sample_fwd_call(shape, dt=BF16, ids_only=False, pretrain=0, act=None, dev_scalars=False, **state):
    """gic_decoder_sample_fwd over fake pointers; act: host_active_rows of a resumed roll-out (read on the host: a real array)."""
    opts = PL.DecoderSampleOpts()
    opts.no_state = int(ids_only or act is not None)
    keep = []
    if act is not None:
        src, rows = fake(PL.DecoderState()), (ctypes.c_int32 * len(act))(*act)
        opts.resume_from, opts.resume_B, opts.host_active_rows = ctypes.cast(ctypes.pointer(src), ctypes.c_void_p), 2, ctypes.cast(rows, ctypes.c_void_p)
        opts.force_ids = opts.force_len = P
        keep = [src, rows]
    if dev_scalars:
        opts.dev_scalars = P
    out = None if opts.no_state else P
    return ("gic_decoder_sample_fwd", (PL.DecoderDims(*shape, dt), *fake_decoder(shape[5], **state), P, None, 1, 1.0, pretrain, out, P, opts, None)), keep


def test_backward_and_weight_gradient_selection():
    """select_decoder_bwd: lstm_bwd_step's chain needs H % 8 (the forward's H % 8 too: H = 10 is generic in both), every transposed image
    and at most 512 rows -- V and E do not enter it (V = 6: a generic roll-out, a fused backward).  Per layer the weight gradient is one
    folded product where gic_debug_wgrad_fold names a tile width that divides din, else two products and colsum; the deterministic mode
    honours no weight-gradient extras."""
    lib = PL.load()
    path = lambda shape, flags=0, dt=BF16: (lambda s, l: (s, fwd_path(l), bwd_path(l)))(*decoder_plan(*shape, dt=dt, flags=flags | TRAIN))
    assert path(BASE) == (0, "FUSED", "FUSED")
    assert path((2, 3, 6, 8, 8, 1)) == (0, "GENERIC", "FUSED")
    assert path((2, 3, 8, 8, 10, 1)) == (0, "GENERIC", "GENERIC")
    assert path((2, 3, 8, 8, 12, 1)) == (0, "GENERIC", "GENERIC")
    assert path((2, 3, 8, 8, 8, 2), NO_WCAT_T) == (0, "FUSED", "GENERIC")           # one layer of two without its image
    assert path((512, 3, 8, 8, 8, 1)) == (0, "FUSED", "FUSED") and path((513, 3, 8, 8, 8, 1)) == (0, "GENERIC", "GENERIC")
    status, lines = decoder_plan(2, 3, 8, 8, 8, 2, flags=TRAIN | NO_WCAT_T)         # the generic chain: the image where there is one
    chain = [l for l in lines if l.endswith(" x3") and l.startswith("gemm<")][-2:]
    assert chain[0].startswith("gemm<bf16,f32,true,true,") and chain[1].startswith("gemm<bf16,f32,true,false,"), lines
    status, lines = decoder_plan(2, 3, 8, 8, 8, 2, flags=TRAIN | STATE_GRADS)       # d h_-1: one more product per layer
    assert sum(l.endswith("M=2 N=8 K=32 x1") for l in lines) == 2
    # the folded form, from what the library's wgrad query answers: M = 4H, N = din + H, K = B * L
    for (B, Lc, E, H), folded in (((64, 20, 512, 512), True), ((64, 20, 520, 512), False), ((64, 20, 64, 64), True), ((64, 20, 72, 64), False)):
        tn = lib.gic_debug_wgrad_fold(P, P, 4 * H, E + H, B * Lc, 4 * H, E + H, 0, 0, BF16, F32)
        assert tn in (64, 128) and (E % tn == 0) == folded
        for det in (False, True):
            engine.set_deterministic(det)
            try:
                status, lines = decoder_plan(B, Lc, 1000, E, H, flags=TRAIN)
            finally:
                engine.set_deterministic(False)
            tail = lines[lines.index("backward path=FUSED") + 4:]
            if folded and not det:
                assert len(tail) == 1 and f"a_sum=2 n_split={E} M={4 * H} N={E + H} K={B * Lc} x1" in tail[0], tail
            else:
                assert len(tail) == 3 and tail[2] == "colsum x1" and f"M={4 * H} N={E} K={B * Lc} x1" in tail[0] and f"N={H} K={B * Lc} x1" in tail[1]
    # softmax_bwd's variant: 16-byte rows (V % 8 in bf16, V % 4 in f32) and the register budget
    soft = lambda V, dt: next(l for l in decoder_plan(2, 3, V, 8, 8, dt=dt, flags=TRAIN)[1] if l.startswith("softmax")).split()[0]
    assert [soft(V, BF16) for V in (8, 12, 10240, 10248, 16384, 16392)] == ["softmax_bwd_vec_kernel<bf16,5>", "softmax_bwd_kernel<bf16>",
            "softmax_bwd_vec_kernel<bf16,5>", "softmax_bwd_vec_kernel<bf16,8>", "softmax_bwd_vec_kernel<bf16,8>", "softmax_bwd_kernel<bf16>"]
    assert [soft(V, F32) for V in (8, 6, 8192, 8196)] == ["softmax_bwd_vec_kernel<f32,8>", "softmax_bwd_kernel<f32>", "softmax_bwd_vec_kernel<f32,8>",
                                                          "softmax_bwd_kernel<f32>"]
    assert "softmax" not in "".join(decoder_plan(*BASE, flags=TRAIN | PRETRAIN)[1])  # pretrain: d_out is d_logits


def test_row_key_roll_out():
    """DEC_GENERIC_ROWKEY: a bf16 ids-only roll-out off the fused path whose L * 8 key bytes fit a row of V * 4 logits bytes (V % 4) with
    the logits scratch on 8 bytes.  Its steps take the vocabulary product with the Gumbel-max epilogue + rollout_pick from
    gemm_gumbelmax_from_cols rows on (the plan's from=, read from the library), below it the separate product + the argmax kernel; after
    one such step the separate launches stay, whatever a later step's rows (a resumed roll-out whose rows cross the bound upward)."""
    lib = PL.load()
    key = lambda V, Lc=20, dt=BF16, flags=0, B=513: fwd_path(decoder_plan(B, Lc, V, 8, 8, dt=dt, flags=flags)[1])
    assert key(40) == "GENERIC_ROWKEY" and key(36) == "GENERIC" and key(42) == "GENERIC" and key(44, 22) == "GENERIC_ROWKEY" and key(44, 23) == "GENERIC"
    assert key(40, dt=F32) == "GENERIC" and key(40, flags=TRAIN) == "GENERIC" and key(40, flags=PRETRAIN) == "GENERIC" and key(40, flags=LOGITS_4) == "GENERIC"
    assert key(40, B=512) == "FUSED" and key(40, B=512, flags=RESUMED) == "GENERIC_ROWKEY"
    shape = lambda B: (B, 4, 1280, 8, 8, 1)
    status, lines = decoder_plan(*shape(4096))
    bound = int(lines[0].split("from=")[1])
    assert status == 0 and bound == 128 * 15 + 1            # 10 row tiles of the 1280 words: 16 column tiles make 160 tiles of 128 x 128
    assert decoder_plan(2, 4, 40, 8, 8)[1][0] == "forward path=FUSED from=0" and decoder_plan(513, 20, 40, 8, 8)[1][0].endswith("from=0")    # V < 128: never
    status, below = decoder_plan(*shape(bound - 1))
    status, at = decoder_plan(*shape(bound))
    assert [l.split("<")[0] for l in below[2:]] == ["lstm_pointwise_fwd_kernel", "gemm", "gumbel_softmax_argmax_reg_kernel"], below
    assert [l.split("<")[0] for l in at[2:]] == ["lstm_pointwise_fwd_kernel", "tile8", "rollout_pick_kernel"], at
    assert at[3].startswith("tile8<f32,128,3,false,") and f"M=1280 N={bound} K=8 x4" in at[3]        # (3: the Gumbel-max epilogue)
    assert at[4] == f"rollout_pick_kernel<bf16> grid={-(-bound // 4)} block=256 lds=0 x4"
    assert f"M={bound - 1} N=1280 K=8 x4" in below[3] and below[4] == f"gumbel_softmax_argmax_reg_kernel<bf16,1,true> grid={bound - 1} block=1024 lds=0 x4"
    # the entry point in route-only mode walks the call's own rows and selects each step's products: the route line is the last step's
    # vocabulary product -- with the Gumbel-max epilogue (tile8<f32,128,3,..>) where the step took it
    walk = lambda B, act=None, **kw: (lambda c: (route(c[0]), c[1]))(sample_fwd_call(shape(B), ids_only=True, act=act, **kw))[0]
    keyed = lambda r: (r[0], r[1].startswith("tile8<f32,128,3,false,"), r[1].startswith("gemm<bf16,f32,true,true,"))
    assert keyed(walk(bound)) == (0, True, False) and keyed(walk(bound - 1)) == (0, False, True)
    assert keyed(walk(bound, act=[0, bound, bound, bound])) == (0, True, False)
    assert keyed(walk(bound, act=[0, 600, bound, bound])) == (0, False, True)         # declined once: the separate launches from there on
    assert keyed(walk(bound, act=[0, 0, bound, bound])) == (0, True, False)           # (a step without rows declines nothing)
    assert keyed(walk(bound, logits=P + 4)) == (0, False, True)
    assert walk(600, dev_scalars=True)[0] == UNSUPPORTED and lib.gic_last_error() == DEV_SCALARS_REFUSAL
    # gic_attn_rollout likewise, but each step on its own rows (its logits scratch holds only the steps below the bound)
    d = PL.AttnDims(4, 4, 1280, 8, 8, 8, 4, 8, BF16)

    def attn(*rows):
        act = (ctypes.c_int32 * 4)(*rows)
        return route(("gic_attn_rollout", (d, fake(PL.AttnParams()), fake(PL.AttnShadow()), fake(PL.AttnState()), P, P, bound, P,
                                           ctypes.cast(act, ctypes.c_void_p), None, 1, P, P, None)))
    assert keyed(attn(0, 600, bound - 1, bound)) == (0, True, False) and keyed(attn(0, 600, bound - 1, bound - 1)) == (0, False, True)


STEP_TABLE = [(dt, H, din, B) for dt in (BF16, F32) for H, din in ((8, 8), (512, 512), (512, 1536), (40, 24)) for B in (64, 65)]


@pytest.mark.parametrize("dt,H,din,B", STEP_TABLE, ids=lambda v: str(v))
def test_step_launch_plans_equal_the_parents_formulae(dt, H, din, B):
    """select_lstm_step / select_vocab_step against the restated launch-site expressions of the commit before them: H = 8 (the staged tile
    is smaller than the reduction / epilogue scratch), H = 512 with ldx = 1024 and 2048 (the chunk at its 2 KiB / 1 KiB cap in bf16, past
    it in f32), H = 40 (a chunk rounded up to 32 elements), 64 rows against 65 (a second row block), every variant."""
    ldx = din + H
    for variant in (0, 1, 2):
        assert step_plan(1, variant, dt, B, H, ldx) == lstm_line(dt, B, H, ldx, variant)
    for V in (8, 10000):
        assert step_plan(0, 0, dt, B, H, V) == vocab_line(dt, B, V, H, 0)
        assert step_plan(0, 1, dt, B, H, V) == vocab_line(dt, B, V, H, 1)
        for K in (1, 8):
            assert step_plan(0, 2, dt, B, H, V, K) == vocab_line(dt, B, V, H, 2, K)
            assert step_plan(0, 3, dt, B, H, V, K) == vocab_line(dt, B, V, H, 3, K)
        for K in (2, 8):
            assert step_plan(0, 4, dt, B, H, V, K) == vocab_line(dt, B, V, H, 4, K)
    assert lstm_lds(BF16, 16) == 34816 and vocab_lds(BF16, 8) == 20480 and lstm_chunk(BF16, 2048) == 1024 and vocab_chunk(F32, 512) == 256


def sample_bwd_call(shape, dt=BF16, phases=3):
    prm, sh, st = fake_decoder(shape[5])
    return ("gic_decoder_sample_bwd", (PL.DecoderDims(*shape, dt), prm, sh, st, fake(PL.DecoderBwdWs()), P, P, P, 1.0, 0, fake(PL.DecoderGrads()),
                                       phases, None, None))


def test_route_only_decoder_passes_launch_nothing():
    """gic_decoder_sample_fwd / _bwd, the teacher-forced entries and gic_attn_rollout in route-only mode: validated, selected, status
    returned -- over fake pointers, on a machine that may have no GPU at all.  A pass that selects no product of its own leaves the
    route line as it was; validation still comes first."""
    lib = PL.load()
    shape = (64, 20, 10000, 512, 512, 1)
    projection = route(gemm(1280, 10000, 512, 1, 1, F32, F32, 0))[1]
    with engine.route_only() as r:                 # (one context: leaving a nested one would end the mode for the calls behind it)
        lib.gic_gemm(*gemm(64, 512, 2048, 1, 1, BF16, F32, 0)[1])
        line = r.last()
        for dt in (BF16, F32):
            call, keep = sample_fwd_call(shape, dt)
            assert getattr(lib, call[0])(*call[1]) == 0, lib.gic_last_error()
            call = sample_bwd_call(shape, dt)
            assert getattr(lib, call[0])(*call[1]) == 0, lib.gic_last_error()
            d = PL.DecoderDims(64, 21, 10000, 512, 512, 1, dt)
            prm, sh, st = fake_decoder()
            assert lib.gic_decoder_forward_tf_bwd(d, prm, sh, st, fake(PL.DecoderBwdWs()), P, P, P, 20, P, 1.0, 1, fake(PL.DecoderGrads()), None) == 0
        assert r.last() == line
        # the passes with products of their own leave the last one's line: the teacher-forced projection over B * Tmax rows ...
        assert lib.gic_decoder_forward_tf(d, prm, sh, st, P, P, P, 20, None, 1, 1.0, 1, P, P, P, P, P, None) == 0, lib.gic_last_error()
        assert r.last() == projection != line
        # ... and a generic roll-out's last vocabulary product
        call, keep = sample_fwd_call((600, 20, 10000, 512, 512, 1), ids_only=True)
        assert getattr(lib, call[0])(*call[1]) == 0 and r.last().startswith("tile8<f32,128,3,false,"), r.last()
        # ... and validation still comes first
        call, keep = sample_fwd_call(shape)
        assert lib.gic_decoder_sample_fwd(*call[1][:4], None, *call[1][5:]) == INVALID_ARG and lib.gic_last_error() == b"decoder_sample_fwd: null argument"
        call = sample_bwd_call(shape, phases=8)
        assert getattr(lib, call[0])(*call[1]) == INVALID_ARG and lib.gic_last_error() == b"decoder_sample_bwd: phases must be a mask of 1 | 2 | 4"
        call, keep = sample_fwd_call((600, 20, 10000, 512, 512, 1), ids_only=True, gpre=None)
        assert getattr(lib, call[0])(*call[1]) == INVALID_ARG
        assert lib.gic_last_error() == b"decoder_sample_fwd: the unfused path needs state->logits and state->gpre"


@pytest.mark.parametrize("env,rows", [({"GIC_FUSED_ROLLOUT_MAX_ROWS": "7"}, 7), ({"GIC_NO_FUSED_ROLLOUT": "1"}, 0)], ids=["max rows", "switched off"])
def test_the_two_switches_move_every_copy_of_the_predicate(env, rows):
    """GIC_FUSED_ROLLOUT_MAX_ROWS / GIC_NO_FUSED_ROLLOUT are read once per process: a fresh child each.  The forward's path, the backward's,
    the row query and the refusal's text all follow."""
    code = ("import ctypes\n"
            "from gan_image_captioning_amd import _lib as L\n"
            "lib = L.load()\n"
            "def plan(B, flags=1):\n"
            "    out = ctypes.create_string_buffer(4096)\n"
            "    s = lib.gic_debug_decoder_plan(ctypes.byref(L.DecoderDims(B, 3, 8, 8, 8, 1, L.BF16)), flags, out, len(out))\n"
            "    return s, [l.split('path=')[1].split()[0] for l in out.value.decode().splitlines() if 'path=' in l]\n"
            "r = ctypes.c_int32(-1)\n"
            "lib.gic_decoder_fused_rollout_rows(ctypes.byref(L.DecoderDims(1, 1, 8, 8, 8, 1, L.BF16)), ctypes.byref(r))\n"
            "print(r.value, plan(7), plan(8), plan(8, 5), lib.gic_last_error().decode())\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], env={**os.environ, **env, "PYTHONPATH": root}, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    seven = "(0, ['FUSED', 'FUSED'])" if rows else "(0, ['GENERIC', 'GENERIC'])"
    limit = 7 if rows else 512                                # the message names the row limit, whatever switched the kernels off
    assert out.stdout.strip() == (f"{rows} {seven} (0, ['GENERIC', 'GENERIC']) (-2, []) decoder_sample_fwd: device-resident step scalars need the fused "
                                  f"step kernels (state->part, B <= {limit}, V % 4 == 0, E, H % 8 == 0)")
