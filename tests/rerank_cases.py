"""Models with spread for the GPU tests of re-ranking and retrieval (tests/test_gpu_rerank.py, tests/test_gpu_retrieval.py)."""
import torch

G_SHARPEN = 10.0


def spread(gen, sharpen=None):
    """Generator.init_params draws every tensor from U(-0.05, 0.05), the frozen trunk's convolutions and BatchNorm scales included: in
    eval mode (running statistics 0 / 1) each BatchNorm then shrinks its input thirty-fold, every image ends at the same pooled
    features, and the beams' scores lie within rounding of each other.  A test of ranking needs images and beams that differ: the
    trunk is re-drawn He-normal with unit BatchNorm scales, and the output layer is sharpened."""
    from gan_image_captioning_amd.trunk import _BNParams, _ConvParams
    g = torch.Generator().manual_seed(77)
    with torch.no_grad():
        for m in gen.encoder.resnet.modules():
            if isinstance(m, _ConvParams):
                w = m.weight
                fan_in = w[0].numel()
                w.copy_((torch.randn(w.shape, generator=g) * (2.0 / fan_in) ** 0.5).to(w.device))
            elif isinstance(m, _BNParams):
                m.weight.fill_(1.0)
                m.bias.zero_()
        gen.decoder.linear.weight.mul_(G_SHARPEN if sharpen is None else sharpen)
        gen.decoder.linear.bias.mul_(G_SHARPEN if sharpen is None else sharpen)
