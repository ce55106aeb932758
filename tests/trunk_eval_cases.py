"""The convolutions of the inference-mode trunk, as tables: behind tests/test_trunk_eval_cases.py (which pins every case's route and the
tables' coverage without a GPU) and tests/test_gpu_trunk_eval.py (which runs every case on the GPU against fp64).  Nothing here touches
the GPU.

In eval mode TrunkPlan launches every convolution through gic_conv2d with a null statistics pointer (EPI_PLAIN): none of the kernels
that exist under the BatchNorm-sum epilogue only (BNSTATS_ONLY below) is eligible, so inference runs on tile8<..,0,true,..> and on the
4-wave gemm<..,0,true,..> kernel alone.

EVAL_WALKS   (arch, S, N, mode, routes): one eval pass of the whole trunk; `routes` maps a variant key (the route line up to " grid=")
             to the layers that must take it, every layer of the arch exactly once.  mode: bf16 | det (bf16 under
             engine.set_deterministic) | fp32.
PLAIN_CONVS  isolated gic_conv2d(stats = None) launches.  The first group holds, for every variant key that any layer of
             SCAN_ARCHS x SCAN_S x SCAN_N x {bf16, f32} reaches, the layer shape with the fewest output rows that reaches it (ties: the
             shallowest K, then the fewest output channels); the second group the edges the scan does not vary.
A change of the selection's thresholds has to move these tables deliberately: the route test fails for every case that slid onto
another kernel, the coverage test for every variant the scan reaches that no case here runs."""
from typing import Dict, List, NamedTuple, Tuple

import torch

from oracle import cpu_encoder as OE

SCAN_ARCHS = ("resnet18", "resnet50")
SCAN_S = (64, 96, 200, 224, 256)
SCAN_N = (1, 2, 3, 5, 8, 16, 32, 64)
MODES = {"bf16": ("bf16", False), "det": ("bf16", True), "fp32": ("f32", False)}        # mode -> (compute dtype, deterministic)
BNSTATS_ONLY = ("conv_stem", "conv3x3_patch", "conv1x1_stream", "conv1x1_panel", "conv1x1_pix")


class Layer(NamedTuple):
    """One convolution as gic_conv2d is handed it: input map H x W x cin, window k x kw (the stem: 7 x 8 over the zero-bordered NHWC4
    image, pad 0)."""
    name: str
    H: int
    W: int
    cin: int
    cout: int
    k: int
    kw: int
    stride: int
    pad: int

    def out_hw(self):
        return (self.H + 2 * self.pad - self.k) // self.stride + 1, (self.W + 2 * self.pad - self.kw) // self.stride + 1


def trunk_layers(arch: str, S: int) -> List[Layer]:
    """Every convolution of the trunk at image size S, in execution order (TrunkPlan.steps), with the map it reads."""
    h = (S + 6 - 7) // 2 + 1
    out = [Layer("0", S + 6, S + 6, 4, 64, 7, 8, 2, 0)]
    cur = (h + 2 - 3) // 2 + 1
    nxt = cur
    for name, cin, cout, k, stride, pad in OE.layer_specs(arch)[1:]:
        if name.endswith("conv1"):
            cur = nxt                                     # a new block: its input map
            here = cur
        elif name.endswith("downsample.0"):
            here = cur
        else:
            here = nxt
        out.append(Layer(name, here, here, cin, cout, k, k, stride, pad))
        if not name.endswith("downsample.0"):
            nxt = (here + 2 * pad - k) // stride + 1
    return out


def conv_args(l, N: int, dtype: int, A, W, C, stream=None) -> tuple:
    """gic_conv2d's arguments for layer (or PlainConv) `l` without a statistics buffer."""
    return (A, W, C, None, 1, dtype, N, l.H, l.W, l.cin, l.cout, l.k, l.kw, l.stride, l.pad, stream)


def route_key(line: str) -> str:
    return line.split(" grid=")[0]


class EvalWalk(NamedTuple):
    arch: str
    S: int
    N: int
    mode: str
    routes: Dict[str, str]

    @property
    def id(self):
        return f"{self.arch}-{self.S}-{self.N}-{self.mode}"

    def key_of(self) -> Dict[str, str]:
        """layer name -> the variant key it must take"""
        return {name: key for key, names in self.routes.items() for name in names.split()}


class PlainConv(NamedTuple):
    N: int
    H: int
    W: int
    cin: int
    cout: int
    k: int
    kw: int
    stride: int
    pad: int
    dtype: str
    key: str
    why: str = ""

    @property
    def id(self):
        return f"{self.N}x{self.H}x{self.W}x{self.cin}-{self.cout}-k{self.k}x{self.kw}s{self.stride}p{self.pad}-{self.dtype}"

    def out_hw(self):
        return (self.H + 2 * self.pad - self.k) // self.stride + 1, (self.W + 2 * self.pad - self.kw) // self.stride + 1

    def rows(self):
        ho, wo = self.out_hw()
        return self.N * ho * wo


def eval_running(batch: Dict[str, Tuple[torch.Tensor, torch.Tensor]], gamma: Dict[str, torch.Tensor], seed: int):
    """Running statistics and affine scales that can expose a wrong eval formula.  batch: BatchNorm name -> (mean, biased variance) of
    one training pass, f32 on the CPU.  Per channel running_mean = mean (1 + delta), delta ~ U(-0.3, 0.3), running_var = var rho, rho
    log-uniform in [0.25, 4]; in every layer two channels get running_var = 0 (only eps is left under the root), two 1e-6 (eps still
    dominates), one gamma = 0; every other gamma is kept (the init's negative ones included).
    -> name -> (running_mean, running_var, gamma), f32."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name in sorted(batch):
        mean, var = (t.float() for t in batch[name])
        C = mean.numel()
        delta = torch.empty(C).uniform_(-0.3, 0.3, generator=g)
        rho = torch.exp2(torch.empty(C).uniform_(-2.0, 2.0, generator=g))
        rm, rv, ga = mean * (1 + delta), var * rho, gamma[name].float().clone()
        pick = torch.randperm(C, generator=g)[:5]
        rv[pick[0:2]] = 0.0
        rv[pick[2:4]] = 1e-6
        ga[pick[4]] = 0.0
        out[name] = (rm.contiguous(), rv.contiguous(), ga)
    return out


def walk_inputs(arch: str, S: int, N: int):
    """(trunk parameters as oracle.cpu_encoder.make_trunk_params names them, the images of the training pass that supplies the batch
    statistics, the images of the eval pass), the same on every machine."""
    g = torch.Generator().manual_seed(S * 100 + N)
    tp = OE.make_trunk_params(arch, g)
    return tp, torch.randn(N, 3, S, S, generator=g), torch.randn(N, 3, S, S, generator=g)


def cpu_eval_pass(arch: str, S: int, N: int, emulate_bf16: bool, prefix: str = "encoder.resnet."):
    """The eval pass of a walk on the CPU oracle, with running statistics made as the GPU test makes them (from the oracle's own
    training pass on the other images): (formed tensors by name, pooled feature, the running / gamma table)."""
    tp, train_images, eval_images = walk_inputs(arch, S, N)
    stats: dict = {}
    OE.trunk_forward(tp, train_images, arch, training=True, stats_out=stats, emulate_bf16=emulate_bf16)
    names = [OE.bn_name(l[0]) for l in OE.layer_specs(arch)]
    table = eval_running({n: stats[prefix + n] for n in names}, {n: tp[prefix + n + ".weight"] for n in names}, seed=S + N)
    tp = dict(tp)
    running = {}
    for n, (rm, rv, ga) in table.items():
        tp[prefix + n + ".weight"] = ga
        running[prefix + n + ".running_mean"], running[prefix + n + ".running_var"] = rm, rv
    formed: dict = {}
    feat = OE.trunk_forward(tp, eval_images, arch, training=False, running=running, emulate_bf16=emulate_bf16, formed=formed)
    return formed, feat, table


EVAL_WALKS: List[EvalWalk] = [
    # captioning one image: the nine layers on 7 x 7 maps (M = 49) on the 4-wave conv kernel, K = 512 ... 4608
    EvalWalk("resnet50", 224, 1, "bf16", {
        "tile8<bf16,64,0,true,4,false,false,1024>": ("0 4.0.conv1 4.0.conv2 4.0.conv3 4.0.downsample.0 4.1.conv1 4.1.conv2 4.1.conv3 4.2.conv1 4.2.conv2 "
                                                      "4.2.conv3 5.0.conv1 5.0.conv2 5.0.conv3 5.0.downsample.0 5.1.conv1 5.1.conv2 5.1.conv3 5.2.conv1 "
                                                      "5.2.conv2 5.2.conv3 5.3.conv1 5.3.conv2 5.3.conv3 6.0.conv1 6.0.conv2 6.0.conv3 6.0.downsample.0 "
                                                      "6.1.conv1 6.1.conv2 6.1.conv3 6.2.conv1 6.2.conv2 6.2.conv3 6.3.conv1 6.3.conv2 6.3.conv3 6.4.conv1 "
                                                      "6.4.conv2 6.4.conv3 6.5.conv1 6.5.conv2 6.5.conv3 7.0.conv1"),
        "gemm<bf16,bf16,true,true,64,64,true,0,true,true>": "7.0.conv2 7.0.conv3 7.0.downsample.0 7.1.conv1 7.1.conv2 7.1.conv3 7.2.conv1 7.2.conv2 7.2.conv3",
    }),
    # an odd batch, row tails everywhere (245 rows at 7 x 7); tile8<bf16,64,0,true,2> and <128,0,true,4>
    EvalWalk("resnet50", 224, 5, "bf16", {
        "tile8<bf16,64,0,true,2,false,false,1024>": "0",
        "tile8<bf16,64,0,true,4,false,false,1024>": ("4.0.conv1 4.0.conv2 4.1.conv1 4.1.conv2 4.2.conv1 4.2.conv2 5.0.conv1 5.0.conv2 5.0.conv3 "
                                                      "5.0.downsample.0 5.1.conv1 5.1.conv2 5.1.conv3 5.2.conv1 5.2.conv2 5.2.conv3 5.3.conv1 5.3.conv2 "
                                                      "5.3.conv3 6.0.conv1 6.0.conv2 6.0.conv3 6.0.downsample.0 6.1.conv1 6.1.conv2 6.1.conv3 6.2.conv1 "
                                                      "6.2.conv2 6.2.conv3 6.3.conv1 6.3.conv2 6.3.conv3 6.4.conv1 6.4.conv2 6.4.conv3 6.5.conv1 6.5.conv2 "
                                                      "6.5.conv3 7.0.conv1 7.0.conv2 7.0.conv3 7.0.downsample.0 7.1.conv1 7.1.conv2 7.1.conv3 7.2.conv1 "
                                                      "7.2.conv2 7.2.conv3"),
        "tile8<bf16,128,0,true,4,false,false,1024>": "4.0.conv3 4.0.downsample.0 4.1.conv3 4.2.conv3",
    }),
    # basic blocks; both 4-wave conv variants (ring and staged)
    EvalWalk("resnet18", 256, 1, "bf16", {
        "tile8<bf16,64,0,true,4,false,false,1024>": ("0 4.0.conv1 4.0.conv2 4.1.conv1 4.1.conv2 5.0.conv1 5.0.conv2 5.0.downsample.0 5.1.conv1 5.1.conv2 "
                                                      "6.0.conv1 6.0.conv2 6.0.downsample.0 6.1.conv1 6.1.conv2"),
        "gemm<bf16,bf16,true,true,64,64,true,0,true,true>": "7.0.conv1 7.0.conv2 7.1.conv1 7.1.conv2",
        "gemm<bf16,bf16,true,true,64,64,true,0,true,false>": "7.0.downsample.0",
    }),
    # 2 x 2 and 4 x 4 maps: windows that are mostly padding, tiles crossing images; 28 layers on the 4-wave kernel
    EvalWalk("resnet50", 64, 3, "bf16", {
        "tile8<bf16,64,0,true,4,false,false,1024>": ("0 4.0.conv1 4.0.conv2 4.0.conv3 4.0.downsample.0 4.1.conv1 4.1.conv2 4.1.conv3 4.2.conv1 4.2.conv2 "
                                                      "4.2.conv3 5.0.conv1 5.0.conv2 5.0.conv3 5.0.downsample.0 5.1.conv1 5.1.conv2 5.1.conv3 5.2.conv1 "
                                                      "5.2.conv2 5.2.conv3 5.3.conv1 5.3.conv2 5.3.conv3 6.0.conv1"),
        "gemm<bf16,bf16,true,true,64,64,true,0,true,true>": ("6.0.conv2 6.0.downsample.0 6.1.conv1 6.1.conv2 6.2.conv1 6.2.conv2 6.3.conv1 6.3.conv2 6.4.conv1 "
                                                              "6.4.conv2 6.5.conv1 6.5.conv2 7.0.conv1 7.0.conv2 7.0.conv3 7.0.downsample.0 7.1.conv1 7.1.conv2 "
                                                              "7.1.conv3 7.2.conv1 7.2.conv2 7.2.conv3"),
        "gemm<bf16,bf16,true,true,64,64,true,0,true,false>": "6.0.conv3 6.1.conv3 6.2.conv3 6.3.conv3 6.4.conv3 6.5.conv3",
    }),
    # deterministic mode switches nothing in eval: the routes of the bf16 walk
    EvalWalk("resnet50", 224, 1, "det", {
        "tile8<bf16,64,0,true,4,false,false,1024>": ("0 4.0.conv1 4.0.conv2 4.0.conv3 4.0.downsample.0 4.1.conv1 4.1.conv2 4.1.conv3 4.2.conv1 4.2.conv2 "
                                                      "4.2.conv3 5.0.conv1 5.0.conv2 5.0.conv3 5.0.downsample.0 5.1.conv1 5.1.conv2 5.1.conv3 5.2.conv1 "
                                                      "5.2.conv2 5.2.conv3 5.3.conv1 5.3.conv2 5.3.conv3 6.0.conv1 6.0.conv2 6.0.conv3 6.0.downsample.0 "
                                                      "6.1.conv1 6.1.conv2 6.1.conv3 6.2.conv1 6.2.conv2 6.2.conv3 6.3.conv1 6.3.conv2 6.3.conv3 6.4.conv1 "
                                                      "6.4.conv2 6.4.conv3 6.5.conv1 6.5.conv2 6.5.conv3 7.0.conv1"),
        "gemm<bf16,bf16,true,true,64,64,true,0,true,true>": "7.0.conv2 7.0.conv3 7.0.downsample.0 7.1.conv1 7.1.conv2 7.1.conv3 7.2.conv1 7.2.conv2 7.2.conv3",
    }),
    # the parity mode
    EvalWalk("resnet18", 96, 2, "fp32", {
        "gemm<f32,f32,true,true,64,64,true,0,true,true>": ("0 4.0.conv1 4.0.conv2 4.1.conv1 4.1.conv2 5.0.conv1 5.0.conv2 5.1.conv1 5.1.conv2 6.0.conv1 "
                                                            "6.0.conv2 6.1.conv1 6.1.conv2 7.0.conv1 7.0.conv2 7.0.downsample.0 7.1.conv1 7.1.conv2"),
        "gemm<f32,f32,true,true,64,64,true,0,true,false>": "5.0.downsample.0 6.0.downsample.0",
    }),
    # the f32 4-wave conv kernel on every layer, K to 4608
    EvalWalk("resnet50", 224, 1, "fp32", {
        "gemm<f32,f32,true,true,64,64,true,0,true,true>": ("0 4.0.conv2 4.1.conv1 4.1.conv2 4.2.conv1 4.2.conv2 5.0.conv1 5.0.conv2 5.0.downsample.0 5.1.conv1 "
                                                            "5.1.conv2 5.2.conv1 5.2.conv2 5.3.conv1 5.3.conv2 6.0.conv1 6.0.conv2 6.0.conv3 6.0.downsample.0 "
                                                            "6.1.conv1 6.1.conv2 6.1.conv3 6.2.conv1 6.2.conv2 6.2.conv3 6.3.conv1 6.3.conv2 6.3.conv3 6.4.conv1 "
                                                            "6.4.conv2 6.4.conv3 6.5.conv1 6.5.conv2 6.5.conv3 7.0.conv1 7.0.conv2 7.0.conv3 7.0.downsample.0 "
                                                            "7.1.conv1 7.1.conv2 7.1.conv3 7.2.conv1 7.2.conv2 7.2.conv3"),
        "gemm<f32,f32,true,true,64,64,true,0,true,false>": "4.0.conv1 4.0.conv3 4.0.downsample.0 4.1.conv3 4.2.conv3 5.0.conv3 5.1.conv3 5.2.conv3 5.3.conv3",
    }),
]

PLAIN_CONVS: List[PlainConv] = [
    # the scan: N, H, W, cin, cout, k, kw, stride, pad, dtype, key, where the scan met the shape first
    PlainConv(1, 4, 4, 256, 512, 1, 1, 2, 0, "bf16", "gemm<bf16,bf16,true,true,64,64,true,0,true,false>", "resnet18@64 7.0.downsample.0, 4 rows"),
    PlainConv(1, 2, 2, 512, 2048, 1, 1, 1, 0, "bf16", "gemm<bf16,bf16,true,true,64,64,true,0,true,true>", "resnet50@64 7.0.conv3, 4 rows"),
    PlainConv(2, 16, 16, 64, 128, 1, 1, 2, 0, "bf16", "tile8<bf16,64,0,true,4,false,false,1024>", "resnet18@64 5.0.downsample.0, 128 rows"),
    PlainConv(32, 7, 7, 512, 2048, 1, 1, 1, 0, "bf16", "tile8<bf16,128,0,true,4,false,false,1024>", "resnet50@200 7.0.conv3, 1568 rows"),
    PlainConv(64, 6, 6, 256, 1024, 1, 1, 1, 0, "bf16", "tile8<bf16,64,0,true,2,false,false,1024>", "resnet50@96 6.0.conv3, 2304 rows"),
    PlainConv(64, 7, 7, 512, 2048, 1, 1, 1, 0, "bf16", "tile8<bf16,128,0,true,2,false,false,1024>", "resnet50@200 7.0.conv3, 3136 rows"),
    PlainConv(64, 13, 13, 256, 1024, 1, 1, 1, 0, "bf16", "tile8<bf16,128,0,true,1,false,false,1024>", "resnet50@200 6.0.conv3, 10816 rows"),
    PlainConv(32, 102, 102, 4, 64, 7, 8, 2, 0, "bf16", "tile8<bf16,64,0,true,1,false,false,1024>", "resnet18@96 0, 73728 rows"),
    PlainConv(1, 4, 4, 256, 512, 1, 1, 2, 0, "f32", "gemm<f32,f32,true,true,64,64,true,0,true,true>", "resnet18@64 7.0.downsample.0, 4 rows"),
    PlainConv(1, 8, 8, 128, 256, 1, 1, 2, 0, "f32", "gemm<f32,f32,true,true,64,64,true,0,true,false>", "resnet18@64 6.0.downsample.0, 16 rows"),
    PlainConv(32, 7, 7, 512, 2048, 1, 1, 1, 0, "f32", "gemm<f32,f32,true,true,128,128,true,0,true,true>", "resnet50@200 7.0.conv3, 1568 rows"),
    PlainConv(8, 28, 28, 128, 512, 1, 1, 1, 0, "f32", "gemm<f32,f32,true,true,128,128,true,0,true,false>", "resnet50@224 5.0.conv3, 6272 rows"),
    # edges the scan does not vary
    PlainConv(1, 7, 7, 512, 512, 3, 3, 1, 1, "bf16", "gemm<bf16,bf16,true,true,64,64,true,0,true,true>", "M = 49 inside a 64-row tile, K = 4608"),
    PlainConv(1, 7, 7, 512, 512, 3, 3, 1, 1, "f32", "gemm<f32,f32,true,true,64,64,true,0,true,true>", "M = 49 inside a 64-row tile, K = 4608"),
    PlainConv(2, 13, 13, 64, 128, 3, 3, 2, 1, "bf16", "gemm<bf16,bf16,true,true,64,64,true,0,true,true>", "stride-2 3x3 on an odd map"),
    PlainConv(2, 13, 13, 64, 128, 3, 3, 2, 1, "f32", "gemm<f32,f32,true,true,64,64,true,0,true,true>", "stride-2 3x3 on an odd map"),
    PlainConv(3, 15, 15, 128, 256, 1, 1, 2, 0, "bf16", "tile8<bf16,64,0,true,4,false,false,1024>", "stride-2 1x1 (downsample) on an odd map"),
    PlainConv(3, 15, 15, 128, 256, 1, 1, 2, 0, "f32", "gemm<f32,f32,true,true,64,64,true,0,true,false>", "stride-2 1x1 (downsample) on an odd map"),
    PlainConv(2, 70, 70, 4, 64, 7, 8, 2, 0, "bf16", "tile8<bf16,64,0,true,4,false,false,1024>", "the stem window 7 x 8 x 4: a 16-byte piece covers two NHWC4 pixels"),
    PlainConv(2, 70, 70, 4, 64, 7, 8, 2, 0, "f32", "gemm<f32,f32,true,true,64,64,true,0,true,true>", "the stem window 7 x 8 x 4: a 16-byte piece covers two NHWC4 pixels"),
    PlainConv(2, 14, 14, 64, 96, 3, 3, 1, 1, "bf16", "tile8<bf16,64,0,true,4,false,false,1024>", "Cout = 96: a ragged second 64-channel tile"),
    PlainConv(2, 14, 14, 64, 96, 3, 3, 1, 1, "f32", "gemm<f32,f32,true,true,64,64,true,0,true,true>", "Cout = 96: a ragged second 64-channel tile"),
    PlainConv(3, 10, 10, 8, 24, 3, 3, 1, 1, "bf16", "tile8<bf16,64,0,true,4,false,false,1024>", "Cout = 24, Cin = 8: one 16-byte piece per tap (bf16)"),
    PlainConv(3, 10, 10, 8, 24, 3, 3, 1, 1, "f32", "gemm<f32,f32,true,true,64,64,true,0,true,false>", "Cout = 24, Cin = 8: one 16-byte piece per tap (bf16)"),
    PlainConv(5, 1, 1, 512, 512, 3, 3, 1, 1, "bf16", "gemm<bf16,bf16,true,true,64,64,true,0,true,true>", "a 1 x 1 map: eight of nine taps are padding, M = 5"),
    PlainConv(5, 1, 1, 512, 512, 3, 3, 1, 1, "f32", "gemm<f32,f32,true,true,64,64,true,0,true,true>", "a 1 x 1 map: eight of nine taps are padding, M = 5"),
    PlainConv(3, 1, 1, 2048, 512, 1, 1, 1, 0, "bf16", "gemm<bf16,bf16,true,true,64,64,true,0,true,true>", "a 1 x 1 map through a 1x1 window, M = 3"),
    PlainConv(3, 1, 1, 2048, 512, 1, 1, 1, 0, "f32", "gemm<f32,f32,true,true,64,64,true,0,true,true>", "a 1 x 1 map through a 1x1 window, M = 3"),
    PlainConv(4, 56, 56, 64, 96, 1, 1, 1, 0, "bf16", "tile8<bf16,64,0,true,4,false,false,1024>", "12544 rows and a ragged channel tile"),
    PlainConv(4, 56, 56, 64, 96, 1, 1, 1, 0, "f32", "gemm<f32,f32,true,true,64,64,true,0,true,false>", "12544 rows and a ragged channel tile"),
    PlainConv(1, 58, 58, 64, 64, 3, 3, 1, 1, "bf16", "tile8<bf16,64,0,true,4,false,false,1024>", "3364 rows (off the 128 grid) under a 3x3 gather"),
    PlainConv(1, 58, 58, 64, 64, 3, 3, 1, 1, "f32", "gemm<f32,f32,true,true,64,64,true,0,true,true>", "3364 rows (off the 128 grid) under a 3x3 gather"),
]
