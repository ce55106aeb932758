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
