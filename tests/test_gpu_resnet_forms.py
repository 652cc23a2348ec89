"""ResNet-18 extractor, the places tests/test_gpu_resnet.py leaves open: every convolution form the network launches (stride 2 and 1x1
with 2 and 4 K steps per tap, even maps, exact / one-row-over / single cut row tiles, maps that are all border), the fp32 -> bf16
roundings bit for bit (the one-product convolution on unrounded input, conv_pack_weight's hi / lo images and the stem's zero columns),
the statistics kernel at its launch-geometry edges (the 2048 switch to the 128-slot form, ragged slot trips, 16 channel groups, one
pixel), the second trip of the two grid-stride loops, every residual block against an fp64 restatement of the recipe the package runs,
BatchNorm under bf16, blank tiles, and the alignment refusals of the C entry points.

The oracle is plain torch in fp64 on the CPU.  Bounds are those of tests/test_gpu_resnet.py (one product of bf16-exact operands 1e-5,
fp32 class 2e-5, statistics / elementwise / average pool 1e-5, max-pool and every rounding exact, whole model 1e-3 absolute in the fp32
class and rel_err 1e-2 in bf16) plus the two block bounds below.

Block bounds (profiles/resnet18_blocks.txt has every figure).  A block is two convolutions and two (three) normalisations.  In the fp32
class, and for layer1 under "bf16" (resnet.BF16_FP32_CLASS), the package is compared with the exact fp64 block: the largest rel_err
measured over the 20 such cases is 1.18e-5, the bound 4 x that; the cap set beforehand is 2e-4, ten per-convolution bounds.  For
layer2 .. 4 under "bf16" it is compared with ref_block(precision="bf16"), which rounds to bf16 what the package rounds -- the weights,
x where it enters conv1 and downsample.0, the post-norm ReLU output where it enters conv2 -- and nothing else: eight of the 12 cases
are at 1e-7 .. 2e-6, the largest is 5.2e-5 (a rounding of the fp32 mid activation that flips against the fp64 one), the bound 4 x
that; the cap set beforehand is 1.5e-3, about half of the 2.6e-3 by which the recipe differs from the exact block at the least.  The
factor 4 is the headroom the convolution bound 2e-5 has over its measured values."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import rel_err
from tests.test_gpu_resnet import (CONV_CASES, _stats64, bfr, conv_input, conv_weight, gpu_conv, make_model, model_case, nhwc,
                                   ref_forward)

pytestmark = pytest.mark.gpu
DEV = "cuda"
_MODELS = {}

FORM_CASES = {
    # name: (B, H, W, cin, cout, k, stride)
    "3x3s2_128_256_even": (2, 8, 10, 128, 256, 3, 2),               # stride 2, 2 K steps per tap, even map: padding on top / left only
    "3x3s2_256_512": (2, 7, 6, 256, 512, 3, 2),                     # stride 2, 4 K steps per tap, 8 column tiles
    "1x1s2_128_256_even": (2, 8, 10, 128, 256, 1, 2),               # KH = 1, 2 K steps
    "1x1s2_256_512": (3, 7, 5, 256, 512, 1, 2),                     # KH = 1, 4 K steps
    "3x3s1_256_256_one_cut_tile": (2, 7, 9, 256, 256, 3, 1),        # M = 126 < 128
    "3x3s1_64_64_exact_tile": (2, 8, 8, 64, 64, 3, 1),              # M = 128: no row is cut
    "3x3s1_64_64_one_row_over": (1, 3, 43, 64, 64, 3, 1),           # M = 129: the second tile holds one row
    "3x3s1_512_512_2x2": (1, 2, 2, 512, 512, 3, 1),                 # layer4 at a 64 x 64 tile: every pixel is a border pixel
    "3x3s2_64_128_1x1": (2, 1, 1, 64, 128, 3, 2),                   # only the centre tap is inside the image
}


# -- 1. convolution forms the network launches --------------------------------------------------------------------------------
@pytest.mark.parametrize("x3", [False, True], ids=["bf16", "x3"])
@pytest.mark.parametrize("name", list(FORM_CASES))
def test_network_conv_forms_against_fp64(name, x3):
    b, h, w_, cin, cout, k, stride = FORM_CASES[name]
    x, w = conv_input((b, cin, h, w_), 1), conv_weight(cout, cin, k, 2)
    if not x3:
        x, w = bfr(x), bfr(w)            # operands pre-rounded: the only error left is the fp32 accumulation
    ref = F.conv2d(x.double(), w.double(), stride=stride, padding=k // 2)
    out = gpu_conv(x, w, k, stride, x3)
    assert tuple(out.shape) == (b, ref.shape[2], ref.shape[3], cout)
    err = rel_err(out.cpu().permute(0, 3, 1, 2), ref)
    print("conv %s %s rel_err %.3e" % (name, "x3" if x3 else "bf16", err))
    assert err < (2e-5 if x3 else 1e-5)
    if not x3:
        assert torch.equal(gpu_conv(x, w, k, stride, False, src_bf16=True), out)


# -- 2. roundings, bit for bit ------------------------------------------------------------------------------------------------
def _ties():
    """bf16 ties and near-ties around 1: nearest-even sends 1 + 2^-8 down to 1 and 1 + 3 2^-8 up to 1 + 2^-6, truncation sends both to
    the lower neighbour, round-half-away both to the upper one; the near-ties are 2^-20 off the tie on either side."""
    t, e = 2.0 ** -8, 2.0 ** -20
    return torch.tensor([1 + t, -(1 + t), 1 + 3 * t, -(1 + 3 * t), 1 + t + e, 1 + t - e, -(1 + t + e), -(1 + t - e)])


def _trunc_bf16(t):
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def _half_away_bf16(t):
    return ((t.contiguous().view(torch.int32) + 0x8000) & -65536).view(torch.float32).to(torch.bfloat16)


@pytest.mark.parametrize("name", ["3x3s2_64_128_straddles_images", "1x1s2_128_256_even"])
def test_one_product_conv_rounds_unrounded_input_to_nearest_even(name):
    """The conversion inside the kernel (fp32 source, hi-only weights) gives the bits of torch's round-to-nearest-even cast."""
    from snuffy_amd import ops
    b, h, w_, cin, cout, k, stride = {**CONV_CASES, **FORM_CASES}[name]
    x, w = conv_input((b, cin, h, w_), 1), conv_weight(cout, cin, k, 2)
    x[0, :8, 0, 0] = _ties()
    assert not torch.equal(bfr(x), x)                                     # unrounded: the conversion has work to do
    hi, lo = ops.conv_pack_weight(w.to(DEV), split=False)
    assert lo is None
    xd = nhwc(x).to(DEV)
    out = ops.conv2d_nhwc(xd, hi, None, k, stride)
    assert torch.equal(out, ops.conv2d_nhwc(xd.to(torch.bfloat16), hi, None, k, stride))
    # the comparison can fail: the other two roundings of the same map, and of the eight ties alone, reach the output
    assert not torch.equal(out, ops.conv2d_nhwc(_trunc_bf16(xd), hi, None, k, stride))
    ties_away = xd.to(torch.bfloat16)
    ties_away[0, 0, 0, :8] = _half_away_bf16(xd[0, 0, 0, :8])
    assert not torch.equal(ties_away, xd.to(torch.bfloat16))
    assert not torch.equal(out, ops.conv2d_nhwc(ties_away, hi, None, k, stride))
    ties_trunc = xd.to(torch.bfloat16)
    ties_trunc[0, 0, 0, :8] = _trunc_bf16(xd[0, 0, 0, :8])
    assert not torch.equal(out, ops.conv2d_nhwc(ties_trunc, hi, None, k, stride))


def _check_weight_images(w, kp):
    from snuffy_amd import ops
    cout = w.shape[0]
    wp = w.permute(0, 2, 3, 1).reshape(cout, -1)                          # the kernels' K order: tap-major, channel-minor
    n = wp.shape[1]
    width = kp if kp is not None else n
    want_hi = torch.zeros(cout, width, dtype=torch.bfloat16)
    want_lo = torch.zeros(cout, width, dtype=torch.bfloat16)
    want_hi[:, :n] = wp.to(torch.bfloat16)
    want_lo[:, :n] = (wp - want_hi[:, :n].float()).to(torch.bfloat16)
    hi, lo = ops.conv_pack_weight(w.to(DEV), split=True, kp=kp)
    assert tuple(hi.shape) == tuple(lo.shape) == (cout, width) and hi.dtype == lo.dtype == torch.bfloat16
    assert torch.equal(hi.cpu().view(torch.int16), want_hi.view(torch.int16))
    assert torch.equal(lo.cpu(), want_lo)
    assert not hi.cpu()[:, n:].view(torch.int16).any() and not lo.cpu()[:, n:].view(torch.int16).any()
    hi1, lo1 = ops.conv_pack_weight(w.to(DEV), split=False, kp=kp)
    assert lo1 is None and torch.equal(hi1, hi)


def test_conv_pack_weight_images_body():
    w = conv_weight(128, 64, 3, 2)
    w[0, :8, 0, 0] = _ties()                                              # ties of the hi image
    t, s = 2.0 ** -10, 2.0 ** -18
    w[5, :4, 2, 1] = torch.tensor([1 + t + s, 1 + t + 3 * s, -(1 + t + s), -(1 + t + 3 * s)])      # hi = +-1: ties of the lo image
    w[127, 63, 2, 2], w[64, 0, 1, 1] = 0.0, -0.0
    _check_weight_images(w, None)


def test_conv_pack_weight_images_stem_zero_padding():
    from snuffy_amd import ops
    assert ops.CONV_STEM_KP == 192
    _check_weight_images(conv_weight(64, 3, 7, 4), ops.CONV_STEM_KP)      # columns 147 .. 191 are zero in both images


# -- 3. statistics kernel at its launch-geometry edges ----------------------------------------------------------------------------
STAT_MAPS = {
    # name: (b, h, w, c)
    "hw2047_last_32_slot_launch": (2, 23, 89, 64),
    "hw2048_first_128_slot_launch": (2, 32, 64, 64),
    "hw2049_ragged_slot_trip_c512": (2, 3, 683, 512),
    "hw33_one_over_a_slot_trip_c512": (3, 1, 33, 512),
    "hw1_zero_variance": (2, 1, 1, 64),
}


def _stat_map(b, h, w_, c):
    """NHWC map whose mean and spread depend on channel and image, so that a channel or an image mix-up shows."""
    g = torch.Generator().manual_seed(20)
    ch, im = torch.arange(c), torch.arange(b).view(b, 1, 1, 1)
    return torch.randn(b, h, w_, c, generator=g) * (0.25 + ch % 5) + 0.3 * (ch % 11) - 1 + 0.5 * im


@pytest.mark.parametrize("name", list(STAT_MAPS))
def test_statistics_and_avgpool_at_geometry_edges(name):
    from snuffy_amd import ops
    b, h, w_, c = STAT_MAPS[name]
    x = _stat_map(b, h, w_, c)
    xd = x.to(DEV)
    mean, rstd = ops.instnorm_stats_nhwc(xd)
    avg = ops.avgpool_nhwc(xd)
    assert tuple(mean.shape) == tuple(rstd.shape) == tuple(avg.shape) == (b, c)
    m0, r0 = _stats64(x.permute(0, 3, 1, 2))
    e_m, e_r, e_a = rel_err(mean.cpu(), m0), rel_err(rstd.cpu(), r0), rel_err(avg.cpu(), m0)
    print("stats %s mean %.3e rstd %.3e avgpool %.3e" % (name, e_m, e_r, e_a))
    assert e_m < 1e-5 and e_r < 1e-5 and e_a < 1e-5
    if h * w_ == 1:
        assert rel_err(rstd.cpu(), torch.full((b, c), 1.0 / math.sqrt(1e-5), dtype=torch.float64)) < 1e-5
        assert torch.equal(mean.cpu(), x.view(b, c)) and torch.equal(avg.cpu(), x.view(b, c))


# -- 4. second trip of the grid-stride loops --------------------------------------------------------------------------------------
def test_norm_act_second_grid_trip():
    """[2, 129, 128, 256]: 1 056 768 float4 groups per image, 4096 x 256 = 1 048 576 of them (rows 0 .. 127) in the first trip."""
    from snuffy_amd import ops
    b, c, h, w_ = 2, 256, 129, 128
    assert h * w_ * c // 4 > 4096 * 256 and 128 * w_ * c // 4 == 4096 * 256
    x = conv_input((b, c, h, w_), 21) * 2.0 + 3.0
    ident = torch.randn(b, c, h, w_, generator=torch.Generator().manual_seed(22))
    xd, idd = nhwc(x).to(DEV), nhwc(ident).to(DEV)
    mean, rstd = ops.instnorm_stats_nhwc(xd)
    ref = torch.relu(F.instance_norm(x.double(), eps=1e-5) + ident.double())
    out = ops.norm_act_nhwc(xd, mean, rstd, identity=idd, relu=True)
    got = out.cpu().permute(0, 3, 1, 2)
    e_all, e_tail = rel_err(got, ref), rel_err(got[:, :, 128:], ref[:, :, 128:])
    print("norm_act second trip: all rows %.3e, rows 128.. %.3e" % (e_all, e_tail))
    assert e_all < 1e-5
    assert e_tail < 1e-5                                                  # the groups only a second trip reaches
    out_bf = ops.norm_act_nhwc(xd, mean, rstd, identity=idd, relu=True, out_dtype=torch.bfloat16)
    assert torch.equal(out_bf, out.to(torch.bfloat16))
    assert torch.equal(out_bf[:, 128:], out[:, 128:].to(torch.bfloat16))
    # constant statistics, gamma and beta (eval-mode BatchNorm)
    g = torch.Generator().manual_seed(23)
    rm, rv = torch.randn(c, generator=g) + 4.0, torch.rand(c, generator=g) + 0.3
    gamma, beta = torch.randn(c, generator=g), torch.randn(c, generator=g)
    ref = torch.relu(F.batch_norm(x.double(), rm.double(), rv.double(), gamma.double(), beta.double(), training=False, eps=1e-5))
    crstd = torch.rsqrt(rv.double() + 1e-5).float()
    out = ops.norm_act_nhwc(xd, rm.to(DEV), crstd.to(DEV), gamma.to(DEV), beta.to(DEV), None, True)
    got = out.cpu().permute(0, 3, 1, 2)
    e_all, e_tail = rel_err(got, ref), rel_err(got[:, :, 128:], ref[:, :, 128:])
    print("norm_act second trip, constant statistics: all rows %.3e, rows 128.. %.3e" % (e_all, e_tail))
    assert e_all < 1e-5
    assert e_tail < 1e-5


def test_maxpool_second_grid_trip():
    """All-negative [1, 514, 514, 64] -> 257 x 257: 1 056 784 float4 groups, the first trip ends one pixel into output row 255."""
    from snuffy_amd import ops
    g = torch.Generator().manual_seed(24)
    x = -(torch.rand(1, 64, 514, 514, generator=g) + 0.1)
    assert 257 * 257 * 16 > 4096 * 256 >= 255 * 257 * 16
    out = ops.maxpool3x3s2_nhwc(nhwc(x).to(DEV))
    assert tuple(out.shape) == (1, 257, 257, 64)
    got, ref = out.cpu().permute(0, 3, 1, 2), F.max_pool2d(x, 3, 2, 1)
    assert torch.equal(got, ref)
    assert torch.equal(got[:, :, 255:], ref[:, :, 255:])                 # the rows a second trip writes


# -- 5. residual blocks against an fp64 restatement of the package's own recipe ---------------------------------------------------
BLOCK_BOUND_FP32_CLASS = 4 * 1.181e-5      # 4 x the largest of the 20 fp32-class cases (layer2.0, instance); cap 2e-4
BLOCK_BOUND_RECIPE = 4 * 5.222e-5          # 4 x the largest of the 12 recipe cases (layer4.0, instance); cap 1.5e-3
assert BLOCK_BOUND_FP32_CLASS < 2e-4 and BLOCK_BOUND_RECIPE < 1.5e-3
BLOCKS = {
    # name: (cin, h, w)
    "layer1.0": (64, 10, 14), "layer1.1": (64, 10, 14),
    "layer2.0": (64, 10, 14), "layer2.1": (128, 5, 7),
    "layer3.0": (128, 10, 14), "layer3.1": (256, 5, 7),
    "layer4.0": (256, 10, 14), "layer4.1": (512, 5, 7),
}


def ref_block(sd, prefix, x, batch, precision):
    """One BasicBlock of ref_forward on x [b, cin, h, w] fp64.  precision="bf16": the package's recipe -- the weights and both activation
    operands of the convolutions whose names do not start with resnet.BF16_FP32_CLASS are rounded to bf16 (x where it enters conv1 and
    downsample.0, the post-norm ReLU output where it enters conv2); the residual x is not, nor anything else."""
    from snuffy_amd import resnet

    def conv(t, name, stride, pad):
        w = sd[name + ".weight"].to(x.dtype)
        if precision == "bf16" and not name.startswith(resnet.BF16_FP32_CLASS):
            t, w = bfr(t), bfr(w)
        return F.conv2d(t, w, stride=stride, padding=pad)

    def norm(t, name):
        if not batch:
            return F.instance_norm(t, eps=1e-5)
        p = [sd["%s.%s" % (name, n)].to(x.dtype) for n in ("running_mean", "running_var", "weight", "bias")]
        return F.batch_norm(t, p[0], p[1], p[2], p[3], training=False, eps=1e-5)

    down = prefix + ".downsample.0.weight" in sd
    stride = 2 if down else 1
    y = torch.relu(norm(conv(x, prefix + ".conv1", stride, 1), prefix + ".bn1"))
    y = norm(conv(y, prefix + ".conv2", 1, 1), prefix + ".bn2")
    identity = norm(conv(x, prefix + ".downsample.0", stride, 0), prefix + ".downsample.1") if down else x
    return torch.relu(y + identity)


def _block_model(norm_layer):
    if norm_layer not in _MODELS:
        model = make_model(norm_layer)
        sd = {k: v.clone() for k, v in model.state_dict().items()}
        _MODELS[norm_layer] = (model.to(DEV).eval(), sd)
    return _MODELS[norm_layer]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("norm_layer", ["instance", "batch"])
@pytest.mark.parametrize("name", list(BLOCKS))
def test_block_against_fp64_recipe(name, norm_layer, precision):
    model, sd = _block_model(norm_layer)
    cin, h, w_ = BLOCKS[name]
    x = conv_input((2, cin, h, w_), 30 + list(BLOCKS).index(name))
    blk = getattr(model, name[:6])[int(name[7])]
    model.configure(precision)
    try:
        with torch.no_grad():
            out = model._block(model._images(), name, blk, nhwc(x).to(DEV))
    finally:
        model.configure("fp32")
    assert out.dtype == torch.float32
    got = out.cpu().permute(0, 3, 1, 2)
    batch = norm_layer == "batch"
    exact = ref_block(sd, name, x.double(), batch, "fp32")
    assert tuple(got.shape) == tuple(exact.shape)
    e_exact = rel_err(got, exact)
    if precision == "fp32" or name.startswith("layer1."):
        print("BLOCK %-8s %-8s %s fp32-class rel_err to the exact block %.3e" % (name, norm_layer, precision, e_exact))
        assert e_exact < BLOCK_BOUND_FP32_CLASS
    else:
        recipe = ref_block(sd, name, x.double(), batch, "bf16")
        e_recipe, gap = rel_err(got, recipe), rel_err(recipe, exact)
        print("BLOCK %-8s %-8s %s recipe rel_err to the restatement %.3e | to the exact block %.3e | restatement to exact %.3e"
              % (name, norm_layer, precision, e_recipe, e_exact, gap))
        assert e_recipe < BLOCK_BOUND_RECIPE
        assert e_exact > e_recipe                                         # the restatement is nearer than the exact block: it is the recipe


# -- 6. whole-network cases ---------------------------------------------------------------------------------------------------
def test_model_batch_norm_bf16():
    """Measured 2.09e-3 (profiles/resnet18_blocks.txt); the fp64 emulation that rounds every convolution's operands gives 2.6e-3."""
    model, x, ref, _ = model_case("batch", 72, 88)
    g = torch.Generator().manual_seed(25)
    u8 = torch.randint(0, 256, (2, 72, 88, 3), generator=g, dtype=torch.uint8)
    model.configure("bf16")
    try:
        out = model(x.to(DEV))
        from_u8 = model.forward_u8(u8.to(DEV))
        from_f32 = model((u8.permute(0, 3, 1, 2).float() / 255).to(DEV))
    finally:
        model.configure("fp32")
    assert tuple(out.shape) == (2, 512) and out.dtype == torch.float32
    err = rel_err(out.cpu(), ref)
    print("MODEL batch bf16 72x88 rel_err %.3e" % err)
    assert err < 1e-2
    assert torch.equal(from_u8, from_f32)


def _blank_tiles():
    white = torch.full((72, 88, 3), 255, dtype=torch.uint8)
    two_tone = torch.full((72, 88, 3), 255, dtype=torch.uint8)
    two_tone[:, 44:] = 51
    two_tone[:, :, 1] //= 2
    return torch.stack([white, two_tone])


def test_blank_tiles():
    """A black tile has zero variance in every InstanceNorm of the network: the features are exactly zero.  White and two-tone tiles
    (constant away from the borders and the seam) stay within the fp32 class's bound and finite in bf16."""
    model, sd = _block_model("instance")
    tiles = _blank_tiles()
    black = torch.zeros(2, 72, 88, 3, dtype=torch.uint8)
    with torch.no_grad():
        ref = ref_forward(sd, (tiles.permute(0, 3, 1, 2).float() / 255).double(), False)
    assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0.1
    try:
        for precision in ("fp32", "bf16"):
            model.configure(precision)
            out = model.forward_u8(black.to(DEV))
            assert bool(torch.isfinite(out).all()) and torch.equal(out, torch.zeros_like(out))
            out = model.forward_u8(tiles.to(DEV))
            assert tuple(out.shape) == (2, 512) and bool(torch.isfinite(out).all())
            err = (out.cpu().double() - ref).abs().amax(1)
            print("blank tiles %s: white max abs err %.3e, two-tone %.3e (|ref| max %.3f)"
                  % (precision, float(err[0]), float(err[1]), float(ref.abs().max())))
            if precision == "fp32":
                assert float(err.max()) < 1e-3
    finally:
        model.configure("fp32")


# -- 7. refusals instead of faults --------------------------------------------------------------------------------------------
def _misaligned(t):
    """A contiguous copy of t (fp32, on the GPU) that starts 4 bytes into its buffer."""
    buf = torch.empty(t.numel() + 8, dtype=torch.float32, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 and t.data_ptr() % 16 == 0
    return v


def test_misaligned_views_are_refused_and_the_error_does_not_stick():
    from snuffy_amd import SnuffyHipError, ops
    x = nhwc(conv_input((2, 64, 6, 5), 26)).to(DEV)
    ident = nhwc(conv_input((2, 64, 6, 5), 27)).to(DEV)
    xm, im = _misaligned(x), _misaligned(ident)
    hi, lo = ops.conv_pack_weight(conv_weight(64, 64, 3, 2).to(DEV), split=True)
    mean, rstd = ops.instnorm_stats_nhwc(x)
    calls = [
        lambda t: ops.conv2d_nhwc(t, hi, lo, 3, 1),
        lambda t: ops.instnorm_stats_nhwc(t)[1],
        lambda t: ops.avgpool_nhwc(t),
        lambda t: ops.norm_act_nhwc(t, mean, rstd, identity=ident, relu=True),
        lambda t: ops.maxpool3x3s2_nhwc(t),
    ]
    for call in calls:
        good = call(x)
        with pytest.raises(SnuffyHipError):
            call(xm)
        assert torch.equal(call(x), good)                                 # the refusal left no error behind
    good = ops.norm_act_nhwc(x, mean, rstd, identity=ident, relu=True)
    with pytest.raises(SnuffyHipError):
        ops.norm_act_nhwc(x, mean, rstd, identity=im, relu=True)
    assert torch.equal(ops.norm_act_nhwc(x, mean, rstd, identity=ident, relu=True), good)
    assert torch.equal(xm, x) and torch.equal(im, ident)
