"""ResNet-18 patch extractor on HIP kernels: the embedder of the reference's SimCLR recipe (compute_feats.py --backbone resnet18
--norm_layer instance; roi.py:318-324 builds the same network): torchvision's resnet18 with InstanceNorm2d (or BatchNorm2d) as the norm
layer and fc = Identity.  Inference only -- the reference freezes the backbone (compute_feats.py:432-433).

The state dict has torchvision's key names in torchvision's order (the reference loads checkpoints by position): conv1.weight, bn1.*,
layer{1..4}.{0,1}.conv1.weight, .bn1.*, .conv2.weight, .bn2.*, and for layer{2..4}.0 downsample.0.weight, downsample.1.* behind bn2.
InstanceNorm2d has neither parameters nor buffers, so with norm_layer="instance" the dict is the 20 convolution weights.

Activations are NHWC on the device.  "fp32" is the package's fp32 class (operands split into bf16 hi + lo, three matrix-core products).
"bf16" rounds the two operands of a convolution to bf16 (one product) from layer2 on and keeps the stem and layer1 in the fp32 class:
rounding every convolution's operands puts the features at 1.1e-2 .. 1.4e-2 of their largest value at 224 x 224 (fp64 emulation, the
stem alone 1.0e-2, layer1 8e-3), outside the package's 1e-2 gate for bf16; with the first five convolutions exact it is 5e-3 .. 6e-3.
Statistics, normalisation, residuals and pools are fp32 in both.
"""
import torch
import torch.nn as nn

from . import functional as SF
from . import ops
from ._ffi import SnuffyHipError

LAYER_PLANES = (64, 128, 256, 512)
BF16_FP32_CLASS = ("conv1", "layer1.")       # convolutions that stay in the fp32 class under precision="bf16" (see above)


class _Conv(nn.Module):
    """Holder of a bias-free Conv2d weight under torchvision's name."""

    def __init__(self, cin, cout, k, stride):
        super().__init__()
        self.kernel_size, self.stride = k, stride
        self.weight = nn.Parameter(torch.empty(cout, cin, k, k), requires_grad=False)
        nn.init.kaiming_normal_(self.weight, mode="fan_out", nonlinearity="relu")      # torchvision's ResNet initialisation


class _InstanceNorm(nn.Module):
    """InstanceNorm2d defaults: eps 1e-5, no affine, no running statistics -- nothing in the state dict."""
    eps = 1e-5


class _BatchNorm(nn.Module):
    """Eval-mode BatchNorm2d: per-channel constants."""
    eps = 1e-5

    def __init__(self, c):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(c), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(c), requires_grad=False)
        self.register_buffer("running_mean", torch.zeros(c))
        self.register_buffer("running_var", torch.ones(c))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))


class BasicBlock(nn.Module):
    def __init__(self, cin, planes, stride, norm):
        super().__init__()
        self.conv1 = _Conv(cin, planes, 3, stride)
        self.bn1 = norm(planes)
        self.conv2 = _Conv(planes, planes, 3, 1)
        self.bn2 = norm(planes)
        self.downsample = None
        if stride != 1 or cin != planes:
            self.downsample = nn.Sequential(_Conv(cin, planes, 1, stride), norm(planes))


class ResNet18(nn.Module):
    """forward(x [B, 3, H, W] f32) / forward_u8(tiles [B, H, W, 3] uint8) -> features [B, 512] f32."""

    num_features = 512

    def __init__(self, norm_layer="instance"):
        super().__init__()
        if norm_layer not in ("instance", "batch"):
            raise ValueError("norm_layer must be 'instance' or 'batch'")
        self.norm_layer = norm_layer
        norm = (lambda c: _InstanceNorm()) if norm_layer == "instance" else _BatchNorm
        self.conv1 = _Conv(3, 64, 7, 2)
        self.bn1 = norm(64)
        cin = 64
        for i, planes in enumerate(LAYER_PLANES):
            stride = 1 if i == 0 else 2
            setattr(self, "layer%d" % (i + 1), nn.Sequential(BasicBlock(cin, planes, stride, norm), BasicBlock(planes, planes, 1, norm)))
            cin = planes
        self.fc = nn.Identity()
        self.precision = "fp32"
        self.max_batch = 128          # images per pass through the network: bounds the fp32 maps (the stem's is 3.2 MB per 224 x 224 image)
        self._cache = None
        for p in self.parameters():
            p.requires_grad = False

    def configure(self, precision="fp32"):
        if precision not in ("fp32", "bf16"):
            raise ValueError("precision must be 'fp32' or 'bf16'")
        self.precision = precision
        return self

    def invalidate(self):
        """Forget the packed weight images: call it after editing parameters through `.data` (an edit that changes neither data_ptr
        nor _version, the keys of the cache)."""
        self._cache = None
        SF.drop_param_caches(self)
        return self

    # -- weight images, made once per model and precision ------------------------------------------------------------
    def _images(self):
        tensors = list(self.parameters()) + list(self.buffers())
        key = (self.precision,) + tuple(SF.param_key(t) for t in tensors)
        if self._cache is not None and self._cache[0] == key:
            return self._cache[1]
        img = {}
        for name, m in self.named_modules():
            if isinstance(m, _Conv):
                split = self.precision == "fp32" or name.startswith(BF16_FP32_CLASS)
                img[name] = ops.conv_pack_weight(m.weight.detach(), split=split, kp=ops.CONV_STEM_KP if m.kernel_size == 7 else None)
            elif isinstance(m, _BatchNorm):
                img[name] = (m.running_mean.float().contiguous(), torch.rsqrt(m.running_var.double() + m.eps).float().contiguous())
        self._cache = (key, img)
        return img

    # -- forward ----------------------------------------------------------------------------------------------------
    def _norm(self, img, name, bn, y, identity=None, relu=True, out_dtype=torch.float32):
        if self.norm_layer == "instance":
            mean, rstd = ops.instnorm_stats_nhwc(y, bn.eps)
            return ops.norm_act_nhwc(y, mean, rstd, None, None, identity, relu, out_dtype)
        mean, rstd = img[name]
        return ops.norm_act_nhwc(y, mean, rstd, bn.weight.detach(), bn.bias.detach(), identity, relu, out_dtype)

    def _block(self, img, name, blk, x):
        # the activation between the two convolutions feeds a convolution only: a one-product conv2 gets it as the bf16 operand it becomes
        mid = torch.bfloat16 if img[name + ".conv2"][1] is None else torch.float32
        y = ops.conv2d_nhwc(x, *img[name + ".conv1"], 3, blk.conv1.stride)
        y = self._norm(img, name + ".bn1", blk.bn1, y, None, True, mid)
        y = ops.conv2d_nhwc(y, *img[name + ".conv2"], 3, 1)
        identity = x
        if blk.downsample is not None:
            d = ops.conv2d_nhwc(x, *img[name + ".downsample.0"], 1, blk.downsample[0].stride)
            identity = self._norm(img, name + ".downsample.1", blk.downsample[1], d, None, False)
        return self._norm(img, name + ".bn2", blk.bn2, y, identity, True)

    def _forward_chunk(self, x, img):
        y = ops.conv_stem(x, *img["conv1"])
        y = self._norm(img, "bn1", self.bn1, y, None, True)
        y = ops.maxpool3x3s2_nhwc(y)
        for i in range(1, 5):
            for j, blk in enumerate(getattr(self, "layer%d" % i)):
                y = self._block(img, "layer%d.%d" % (i, j), blk, y)
        return ops.avgpool_nhwc(y)

    def _check(self, h, w):
        for _ in range(5):                       # stem, max-pool, layer2..4: each halves, rounding up
            h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        if self.norm_layer == "instance" and h * w < 2:
            raise ValueError("Expected more than 1 spatial element when training, got input size [.., 512, %d, %d]" % (h, w))

    @torch.no_grad()
    def _run(self, x, b, h, w):
        if not x.is_cuda:
            raise SnuffyHipError("input must be a GPU tensor: snuffy_amd has no CPU fallback")
        self._check(h, w)
        img = self._images()
        step = max(1, int(self.max_batch))
        if b <= step:
            return self._forward_chunk(x, img)
        return torch.cat([self._forward_chunk(x[i:i + step], img) for i in range(0, b, step)])

    def forward(self, x):
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("ResNet18: input must be [B, 3, H, W], got %s" % (tuple(x.shape),))
        return self._run(x.float(), x.shape[0], x.shape[2], x.shape[3])

    def forward_u8(self, tiles):
        """Decoded tiles [B, H, W, 3] uint8; the stem reads value / 255 (ToTensor) itself: same features as forward(to_tensor(tiles))."""
        if tiles.dim() != 4 or tiles.shape[3] != 3 or tiles.dtype != torch.uint8:
            raise ValueError("ResNet18.forward_u8: input must be uint8 [B, H, W, 3], got %s %s" % (tiles.dtype, tuple(tiles.shape)))
        return self._run(tiles, tiles.shape[0], tiles.shape[1], tiles.shape[2])


def resnet18(norm_layer="instance"):
    return ResNet18(norm_layer=norm_layer)
