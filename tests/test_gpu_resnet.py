"""ResNet-18 SimCLR patch extractor on the GPU: every convolution form, the InstanceNorm statistics, the norm / residual / ReLU kernel, the
pools, the whole network in both precisions and both norm layers, and compute_feats end to end.

The oracle is a plain-torch restatement (F.conv2d, F.instance_norm, F.batch_norm, F.max_pool2d, mean) run in fp64 on the CPU.  Conv
inputs are relu(randn) + 0.5 -- a non-zero mean, so that a padding or a variance mistake shows -- and weights kaiming_normal.

Bounds.  A product of bf16-exact operands accumulated in fp32: rel_err < 1e-5 (as test_patchify_exact).  The fp32 class (hi hi + hi lo +
lo hi): < 2e-5.  Statistics: 1e-5, and 1e-4 with the conv input shifted by +50.  The elementwise kernels and the average pool are a
handful of fp32 roundings (2^-24 each) on O(1) values: 1e-5.  The max-pool is exact.  Whole model: atol 1e-3 in the fp32 class; bf16
rel_err < 1e-2 at 224 x 224, and on the smaller maps -- where InstanceNorm over 4 .. 9 values amplifies any rounding beyond what a bf16
implementation can hold -- twice the rel_err of an fp64 emulation that rounds only the two operands of every convolution to bf16."""
import argparse
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
_REF = {}


def bfr(t):
    """Round to bf16, keep the dtype."""
    return t.float().to(torch.bfloat16).to(t.dtype)


def conv_input(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.relu(torch.randn(shape, generator=g)) + 0.5


def conv_weight(cout, cin, k, seed):
    torch.manual_seed(seed)
    return torch.nn.init.kaiming_normal_(torch.empty(cout, cin, k, k), mode="fan_out", nonlinearity="relu")


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def gpu_conv(x, w, k, stride, x3, src_bf16=False):
    from snuffy_amd import ops
    hi, lo = ops.conv_pack_weight(w.to(DEV), split=x3)
    xd = nhwc(x).to(DEV)
    if src_bf16:
        xd = xd.to(torch.bfloat16)
    return ops.conv2d_nhwc(xd, hi, lo, k, stride)


CONV_CASES = {
    # name: (B, H, W, cin, cout, k, stride)
    "3x3s1_64_64_row_tail_borders": (2, 9, 11, 64, 64, 3, 1),
    "3x3s2_64_128_straddles_images": (3, 9, 11, 64, 128, 3, 2),
    "1x1s2_64_128": (3, 9, 11, 64, 128, 1, 2),
    "3x3s1_512_512_longest_k": (3, 3, 3, 512, 512, 3, 1),
    "3x3s1_128_256_two_row_tiles": (2, 13, 11, 128, 256, 3, 1),     # M = 286: three row tiles, the last one cut
}


@pytest.mark.parametrize("x3", [False, True], ids=["bf16", "x3"])
@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv_forms_against_fp64(name, x3):
    b, h, w_, cin, cout, k, stride = CONV_CASES[name]
    x, w = conv_input((b, cin, h, w_), 1), conv_weight(cout, cin, k, 2)
    if not x3:
        x, w = bfr(x), bfr(w)            # operands pre-rounded: the only error left is the fp32 accumulation
    ref = F.conv2d(x.double(), w.double(), stride=stride, padding=k // 2)
    out = gpu_conv(x, w, k, stride, x3)
    assert tuple(out.shape) == (b, ref.shape[2], ref.shape[3], cout)
    err = rel_err(out.cpu().permute(0, 3, 1, 2), ref)
    print("conv %s %s rel_err %.3e" % (name, "x3" if x3 else "bf16", err))
    assert err < (2e-5 if x3 else 1e-5)
    if not x3:                           # the bf16 source is the same operand, already rounded
        assert torch.equal(gpu_conv(x, w, k, stride, False, src_bf16=True), out)


def _stem_inputs():
    g = torch.Generator().manual_seed(3)
    u8 = torch.randint(0, 256, (2, 23, 18, 3), generator=g, dtype=torch.uint8)
    return u8, u8.permute(0, 3, 1, 2).float() / 255, conv_weight(64, 3, 7, 4)


@pytest.mark.parametrize("x3", [False, True], ids=["bf16", "x3"])
def test_stem_against_fp64_and_uint8_entry(x3):
    from snuffy_amd import ops
    u8, x, w = _stem_inputs()
    hi, lo = ops.conv_pack_weight(w.to(DEV), split=x3, kp=ops.CONV_STEM_KP)
    out = ops.conv_stem(x.to(DEV), hi, lo)
    assert tuple(out.shape) == (2, 12, 9, 64)
    xr, wr = (x, w) if x3 else (bfr(x), bfr(w))
    ref = F.conv2d(xr.double(), wr.double(), stride=2, padding=3)
    err = rel_err(out.cpu().permute(0, 3, 1, 2), ref)
    print("stem %s rel_err %.3e" % ("x3" if x3 else "bf16", err))
    assert err < (2e-5 if x3 else 1e-5)
    assert torch.equal(ops.conv_stem(u8.to(DEV), hi, lo), out)          # decoded tiles: value / 255 in the kernel, the same bits


def _stats64(y):
    """mean, rstd [b, c] of y [b, c, h, w] (fp64), InstanceNorm2d's: biased variance, eps 1e-5."""
    y = y.double().flatten(2)
    return y.mean(2), 1.0 / torch.sqrt(y.var(2, unbiased=False) + 1e-5)


@pytest.mark.parametrize("shift,bound", [(0.0, 1e-5), (50.0, 1e-4)], ids=["plain", "shifted50"])
def test_instance_statistics_after_conv(shift, bound):
    """30 pixels per image (a row tile straddles the three images); shifted: the channel mean is large against its spread."""
    from snuffy_amd import ops
    b, h, w_, cin, cout, k, stride = CONV_CASES["3x3s2_64_128_straddles_images"]
    x, w = conv_input((b, cin, h, w_), 1) + shift, conv_weight(cout, cin, k, 2)
    y = gpu_conv(x, w, k, stride, True)
    mean, rstd = ops.instnorm_stats_nhwc(y)
    # the statistics kernel alone: against fp64 statistics of the map it read
    m0, r0 = _stats64(y.cpu().permute(0, 3, 1, 2))
    e_m0, e_r0 = rel_err(mean.cpu(), m0), rel_err(rstd.cpu(), r0)
    # and the chain: against fp64 statistics of the fp64 convolution
    m1, r1 = _stats64(F.conv2d(x.double(), w.double(), stride=stride, padding=1))
    e_m1, e_r1 = rel_err(mean.cpu(), m1), rel_err(rstd.cpu(), r1)
    print("stats shift %g: kernel mean %.3e rstd %.3e | chain mean %.3e rstd %.3e" % (shift, e_m0, e_r0, e_m1, e_r1))
    assert max(e_m0, e_r0) < 1e-5
    assert max(e_m1, e_r1) < bound


def test_instance_statistics_2x2_map():
    from snuffy_amd import ops
    y = conv_input((3, 64, 2, 2), 5) * 3.0
    mean, rstd = ops.instnorm_stats_nhwc(nhwc(y).to(DEV))
    m0, r0 = _stats64(y)
    assert rel_err(mean.cpu(), m0) < 1e-5 and rel_err(rstd.cpu(), r0) < 1e-5


def test_norm_residual_relu_against_instance_norm():
    from snuffy_amd import ops
    x = conv_input((3, 128, 5, 6), 6) * 2.0 + 3.0
    ident = torch.randn(3, 128, 5, 6, generator=torch.Generator().manual_seed(7))
    xd, idd = nhwc(x).to(DEV), nhwc(ident).to(DEV)
    mean, rstd = ops.instnorm_stats_nhwc(xd)
    n64 = F.instance_norm(x.double(), eps=1e-5)
    for identity, relu in ((None, False), (None, True), (idd, True)):
        ref = n64 + (ident.double() if identity is not None else 0.0)
        ref = torch.relu(ref) if relu else ref
        out = ops.norm_act_nhwc(xd, mean, rstd, identity=identity, relu=relu)
        assert rel_err(out.cpu().permute(0, 3, 1, 2), ref) < 1e-5
        out_bf = ops.norm_act_nhwc(xd, mean, rstd, identity=identity, relu=relu, out_dtype=torch.bfloat16)
        assert torch.equal(out_bf, out.to(torch.bfloat16))


def test_norm_constant_statistics_against_batch_norm():
    from snuffy_amd import ops
    g = torch.Generator().manual_seed(8)
    c = 64
    x = conv_input((2, c, 7, 5), 9)
    rm, rv = torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.3
    gamma, beta = torch.randn(c, generator=g), torch.randn(c, generator=g)
    ref = torch.relu(F.batch_norm(x.double(), rm.double(), rv.double(), gamma.double(), beta.double(), training=False, eps=1e-5))
    rstd = torch.rsqrt(rv.double() + 1e-5).float()
    out = ops.norm_act_nhwc(nhwc(x).to(DEV), rm.to(DEV), rstd.to(DEV), gamma.to(DEV), beta.to(DEV), None, True)
    assert rel_err(out.cpu().permute(0, 3, 1, 2), ref) < 1e-5


def test_maxpool_all_negative_map_and_avgpool():
    from snuffy_amd import ops
    g = torch.Generator().manual_seed(10)
    x = -(torch.rand(2, 64, 7, 9, generator=g) + 0.1)                    # zero padding would win everywhere along the border
    out = ops.maxpool3x3s2_nhwc(nhwc(x).to(DEV))
    assert torch.equal(out.cpu().permute(0, 3, 1, 2), F.max_pool2d(x, 3, 2, 1))
    x = conv_input((3, 128, 7, 9), 11)
    avg = ops.avgpool_nhwc(nhwc(x).to(DEV))
    assert rel_err(avg.cpu(), x.double().mean((2, 3))) < 1e-5


# -- whole model ------------------------------------------------------------------------------------------------------------
def ref_forward(sd, x, batch, emulate_bf16=False):
    """torchvision's resnet18 forward with fc = Identity, restated on a state dict; emulate_bf16 rounds the two operands of every
    convolution to bf16 and keeps everything else in the dtype of x."""
    def conv(t, name, stride, pad):
        w = sd[name + ".weight"].to(x.dtype)
        if emulate_bf16:
            t, w = bfr(t), bfr(w)
        return F.conv2d(t, w, stride=stride, padding=pad)

    def norm(t, name):
        if not batch:
            return F.instance_norm(t, eps=1e-5)
        p = [sd["%s.%s" % (name, n)].to(x.dtype) for n in ("running_mean", "running_var", "weight", "bias")]
        return F.batch_norm(t, p[0], p[1], p[2], p[3], training=False, eps=1e-5)

    t = F.max_pool2d(torch.relu(norm(conv(x, "conv1", 2, 3), "bn1")), 3, 2, 1)
    for layer in (1, 2, 3, 4):
        for blk in (0, 1):
            p = "layer%d.%d" % (layer, blk)
            stride = 2 if (layer > 1 and blk == 0) else 1
            y = torch.relu(norm(conv(t, p + ".conv1", stride, 1), p + ".bn1"))
            y = norm(conv(y, p + ".conv2", 1, 1), p + ".bn2")
            if p + ".downsample.0.weight" in sd:
                t = norm(conv(t, p + ".downsample.0", stride, 0), p + ".downsample.1")
            t = torch.relu(y + t)
    return t.mean((2, 3))


def make_model(norm_layer):
    from snuffy_amd.resnet import ResNet18
    torch.manual_seed(0)
    model = ResNet18(norm_layer)
    if norm_layer == "batch":
        g = torch.Generator().manual_seed(12)
        for k, v in model.state_dict().items():
            if k.endswith("running_mean") or k.endswith("bias"):
                v.copy_(0.3 * torch.randn(v.shape, generator=g))
            elif k.endswith("running_var"):
                v.copy_(torch.rand(v.shape, generator=g) + 0.5)
            elif k.endswith("bn1.weight") or k.endswith("bn2.weight") or k.endswith("downsample.1.weight"):
                v.copy_(torch.rand(v.shape, generator=g) + 0.5)
    return model


def model_case(norm_layer, h, w):
    """(model on the GPU, input, fp64 features, fp64 features of the bf16-operand emulation), computed once."""
    key = (norm_layer, h, w)
    if key not in _REF:
        model = make_model(norm_layer)
        sd = {k: v.clone() for k, v in model.state_dict().items()}
        x = conv_input((2, 3, h, w), 13)
        with torch.no_grad():
            ref = ref_forward(sd, x.double(), norm_layer == "batch")
            emu = ref_forward(sd, x.double(), norm_layer == "batch", emulate_bf16=True) if norm_layer == "instance" else None
        _REF[key] = (model.to(DEV).eval(), x, ref, emu)
    return _REF[key]


@pytest.mark.parametrize("h,w", [(64, 64), (72, 88), (224, 224)])
def test_model_fp32_class(h, w):
    model, x, ref, _ = model_case("instance", h, w)
    out = model.configure("fp32")(x.to(DEV))
    assert tuple(out.shape) == (2, 512) and out.dtype == torch.float32
    err = float((out.cpu().double() - ref).abs().max())
    print("model fp32 %dx%d max abs err %.3e (|ref| max %.3f)" % (h, w, err, float(ref.abs().max())))
    assert err < 1e-3


@pytest.mark.parametrize("h,w", [(64, 64), (72, 88), (224, 224)])
def test_model_bf16(h, w):
    """Measured (profiles/resnet18.txt): 4.9e-3 at 224 x 224, 1.5e-2 at 72 x 88, 7.6e-2 at 64 x 64, where the emulation that rounds the
    operands of every convolution gives 1.35e-2, 2.4e-2 and 6.9e-2: the package keeps the stem and layer1 in the fp32 class."""
    model, x, ref, emu = model_case("instance", h, w)
    out = model.configure("bf16")(x.to(DEV))
    model.configure("fp32")
    err, emu_err = rel_err(out.cpu(), ref), rel_err(emu, ref)
    bound = 1e-2 if (h, w) == (224, 224) else 2 * emu_err
    print("model bf16 %dx%d rel_err %.3e (emulation %.3e, bound %.3e)" % (h, w, err, emu_err, bound))
    assert err < bound


def test_model_batch_norm_fp32_class():
    model, x, ref, _ = model_case("batch", 72, 88)
    out = model.configure("fp32")(x.to(DEV))
    err = float((out.cpu().double() - ref).abs().max())
    print("model batch fp32 72x88 max abs err %.3e (|ref| max %.3f)" % (err, float(ref.abs().max())))
    assert err < 1e-3


def test_model_sub_batches_and_uint8_entry():
    """Passing the batch through in chunks changes nothing, and the uint8 entry gives the features of forward(tiles / 255)."""
    model, _, _, _ = model_case("instance", 64, 64)
    g = torch.Generator().manual_seed(14)
    u8 = torch.randint(0, 256, (5, 64, 64, 3), generator=g, dtype=torch.uint8)
    x = (u8.permute(0, 3, 1, 2).float() / 255).to(DEV)      # divided on the host, as ToTensor does (a true division)
    model.configure("fp32")
    whole = model(x)
    assert torch.equal(model.forward_u8(u8.to(DEV)), whole)
    model.max_batch = 2
    try:
        assert torch.equal(model(x), whole)
        assert torch.equal(model.forward_u8(u8.to(DEV)), whole)
    finally:
        model.max_batch = 128


def test_small_input_raises():
    from snuffy_amd import SnuffyHipError
    from snuffy_amd.resnet import ResNet18
    model, _, _, _ = model_case("instance", 64, 64)
    with pytest.raises(ValueError):
        model(torch.zeros(1, 3, 32, 32, device=DEV))                     # layer4 would be 1 x 1: instance_norm refuses
    with pytest.raises(SnuffyHipError):
        ResNet18()(torch.zeros(1, 3, 64, 64))


def test_determinism():
    b, h, w_, cin, cout, k, stride = CONV_CASES["3x3s2_64_128_straddles_images"]
    x, w = conv_input((b, cin, h, w_), 1), conv_weight(cout, cin, k, 2)
    assert torch.equal(gpu_conv(x, w, k, stride, True), gpu_conv(x, w, k, stride, True))
    model, x, _, _ = model_case("instance", 72, 88)
    for precision in ("fp32", "bf16"):
        model.configure(precision)
        assert torch.equal(model(x.to(DEV)), model(x.to(DEV)))
    model.configure("fp32")


def test_invalidate_after_data_edit():
    model, x, _, _ = model_case("instance", 64, 64)
    model.configure("fp32")
    before = model(x.to(DEV))
    w = model.layer4[1].conv2.weight
    saved = w.data.clone()
    try:
        w.data.add_(0.01 * torch.randn_like(saved))
        assert torch.equal(model(x.to(DEV)), before)                     # an edit through .data is invisible to the cache key ...
        model.invalidate()
        assert not torch.equal(model(x.to(DEV)), before)                 # ... until invalidate() says so
    finally:
        w.data.copy_(saved)
        model.invalidate()
    assert torch.equal(model(x.to(DEV)), before)


def test_compute_feats_end_to_end(tmp_path):
    """Tile directory -> SimCLR-shaped weights file -> ResNet-18 embedder -> CSV (%.4f), device-preprocess and host ToTensor paths."""
    import pandas as pd
    from PIL import Image

    from snuffy_amd import compute_feats as cf
    rng = np.random.RandomState(0)
    bag_dir = tmp_path / "single" / "tumor" / "slide_001"
    bag_dir.mkdir(parents=True)
    for r in range(3):
        for c in range(3):
            Image.fromarray(rng.randint(0, 255, (64, 64, 3), dtype=np.uint8)).save(bag_dir / f"{r}_{c}-17.jpeg", quality=95)
    args = argparse.Namespace(backbone="resnet18", norm_layer="instance", embedder="SimCLR", num_classes=1, batch_size=4, num_workers=0,
                              transform=0, dataset="camelyon16", weights=None, precision="fp32")
    torch.manual_seed(1)
    backbone, nf = cf.get_embedder_backbone(args)
    assert nf == 512
    g = torch.Generator().manual_seed(2)
    ck = OrderedDict(("features.%d" % i, v + 0.01 * torch.randn(v.shape, generator=g))
                     for i, v in enumerate(backbone.state_dict().values()))
    for name, shape in (("l1.weight", (512, 512)), ("l1.bias", (512,)), ("l2.weight", (256, 512)), ("l2.bias", (256,))):
        ck[name] = torch.randn(shape, generator=g)
    args.weights = str(tmp_path / "simclr.pth")
    torch.save(ck, args.weights)
    embedder, _ = cf.get_embedder(args, backbone, nf)
    assert torch.equal(embedder.feature_extractor.layer4[1].conv2.weight.cpu(), ck["features.19"])
    labels = {os.path.join("tumor", "slide_001", f"{r}_{c}-17.jpeg"): int((r + c) % 2) for r in range(3) for c in range(3)}
    feats = {}
    for dp in (1, 0):
        args.device_preprocess = dp
        cf.compute_feats(args, [str(bag_dir)], embedder, str(tmp_path / ("out%d" % dp)), labels)
        df = pd.read_csv(tmp_path / ("out%d" % dp) / "single" / "tumor" / "slide_001.csv")
        assert df.shape == (9, 512 + 2) and list(df.columns[-2:]) == ["label", "position"]
        feats[dp] = df.iloc[:, :512].to_numpy()
    files = sorted(str(p) for p in bag_dir.glob("*.jpeg"))
    tf = cf.TileTransform(None)
    x = torch.stack([tf({"input": Image.open(f), "label": 0, "position": None})["input"] for f in files]).to(DEV)
    with torch.no_grad():
        direct, _ = embedder(x)
    np.testing.assert_allclose(feats[1], direct.cpu().numpy(), atol=5.1e-5)
    np.testing.assert_allclose(feats[0], direct.cpu().numpy(), atol=5.1e-5)
    np.testing.assert_allclose(feats[1], feats[0], atol=1e-3)
