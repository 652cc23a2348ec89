"""DINO and MAE training augmentations on the device (csrc/augment.hip), bit-identical to the reference's per-crop PIL chain
(main_dino_adapter.py:674-745 DataAugmentationDINO; main_pretrain_adapter.py: RandomResizedCrop + flip + normalise).

Decoded uint8 tiles [B, H, W, 3] stay on the GPU.  One launch draws a parameter record per (view, image) from Philox
(snf_augment_draw), one launch per view size turns tiles + records into normalised fp32 crops (snf_augment_apply_u8): crop ->
bicubic resize -> flip -> colour jitter -> grayscale -> Gaussian blur -> solarise -> ToTensor + Normalize, every stage in Pillow's
8-bit arithmetic.  Nothing is read back to the host.

Host side here: the record layout, the per-view policies, and pure-host restatements of the two pieces of Pillow arithmetic the
kernels rebuild per record on the device (bicubic_coeffs, gaussian_box_radius) -- the CPU tests pin them against Pillow."""
import ctypes
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _ffi, ops
from .tiles import IMAGENET_MEAN, IMAGENET_STD, PRECISION_BITS, resample_coeffs

# documented bounds of snf_augment_apply_u8; a tile with max(H, W) <= MAX_RATIO * S keeps every crop's reduction <= 8 (ksize <= 33)
MAX_SIZE, MAX_SOURCE, MAX_RATIO, MAX_BLUR_RADIUS, MAX_VIEWS = 256, 1024, 8, 16.0, 16
RECORD_WORDS, POLICY_WORDS = 16, 20
OPS = ("brightness", "contrast", "saturation", "hue")
# the log-aspect interval of RandomResizedCrop as the literals the draw kernel holds
LOG_RATIO_LO, LOG_RATIO_HI = -0.2876820724517809, 0.28768207245178085
# Philox blocks of one record (counter word 1): the ten crop tries, then flags, then blur / permutation, then the factors
DRAW_TRIES, BLOCK_FLAGS, BLOCK_MISC, BLOCK_FACTORS = 10, 10, 11, 12

# one record = 16 little-endian 32-bit words; the table is an int32 [..., 16] tensor on the device
RECORD_DTYPE = np.dtype([("top", "<i4"), ("left", "<i4"), ("ch", "<i4"), ("cw", "<i4"), ("flip", "<i4"), ("jitter", "<i4"),
                         ("order", "<i4"), ("gray", "<i4"), ("brightness", "<f4"), ("contrast", "<f4"), ("saturation", "<f4"),
                         ("hue", "<f4"), ("blur", "<f4"), ("solarize", "<i4"), ("fallback", "<i4"), ("pad", "<i4")])
assert RECORD_DTYPE.itemsize == 4 * RECORD_WORDS


def _cubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def bicubic_coeffs(in_size, out_size):
    """(bounds [out, 2] int32 = (first input pixel, count), coefficients [out, ksize] int32, ksize) of Pillow's 8-bit bicubic
    resampler for in_size -> out_size: tiles.resample_coeffs with support 2 * filterscale and the cubic (a = -0.5) filter."""
    return resample_coeffs(in_size, out_size, _cubic, 2.0)


def max_ksize(h, w, size):
    """Width of the coefficient rows the apply kernel reserves: the ksize of the largest crop an h x w tile allows."""
    scale = max(1.0, max(h, w) / size)
    return int(math.ceil(2.0 * scale)) * 2 + 1


def gaussian_box_radius(radius):
    """(R, ww, fw): the extended-box radius of Pillow's GaussianBlur(radius) (three box passes per direction), in float32 as
    Pillow computes it, and the 24-bit fixed-point weights of a window pixel (ww) and of the two pixels just outside (fw)."""
    f = np.float32
    sigma2 = f(f(f(radius) * f(radius)) / f(3))
    big_l = f(np.sqrt(np.float64(12.0) * np.float64(sigma2) + 1.0))
    l = f(np.floor((np.float64(big_l) - 1.0) / 2.0))
    a = f(f(f(2) * l + f(1)) * f(f(l * f(l + f(1))) - f(f(3) * sigma2)))
    a = f(a / f(f(6) * f(sigma2 - f(f(l + f(1)) * f(l + f(1))))))
    r = f(l + a)
    ww = int(f(f(1 << 24) / f(f(r * f(2)) + f(1))))
    fw = ((1 << 24) - (2 * int(r) + 1) * ww) // 2
    return float(r), ww, fw


@dataclass(frozen=True)
class AugmentPolicy:
    """The distribution of one view's records.  jitter = (brightness, contrast, saturation, hue) half-widths."""
    size: int
    scale: tuple
    p_flip: float = 0.5
    p_jitter: float = 0.8
    jitter: tuple = (0.4, 0.4, 0.2, 0.1)
    p_gray: float = 0.2
    p_blur: float = 0.0
    blur: tuple = (0.1, 2.0)
    p_solarize: float = 0.0

    def row(self):
        """The POLICY_WORDS doubles the draw kernel reads."""
        b, c, s, h = self.jitter
        row = [self.scale[0], self.scale[1], self.p_flip, self.p_jitter, 1.0 - b, 1.0 + b, 1.0 - c, 1.0 + c, 1.0 - s, 1.0 + s,
               -h, h, self.p_gray, self.p_blur, self.blur[0], self.blur[1], self.p_solarize]
        return [float(v) for v in row] + [0.0] * (POLICY_WORDS - len(row))


def dino_policies(global_size=224, local_size=96, local_crops_number=8, global_scale=(0.4, 1.0), local_scale=(0.05, 0.4)):
    """DataAugmentationDINO's three transforms as data: global view 1, global view 2, the local views."""
    return ([AugmentPolicy(global_size, tuple(global_scale), p_blur=1.0),
             AugmentPolicy(global_size, tuple(global_scale), p_blur=0.1, p_solarize=0.2)] +
            [AugmentPolicy(local_size, tuple(local_scale), p_blur=0.5)] * local_crops_number)


def mae_policy(size=224, scale=(0.2, 1.0)):
    return AugmentPolicy(size, tuple(scale), p_jitter=0.0, p_gray=0.0)


def pack_order(names):
    """The record's `order` word for a sequence of the four OPS names: operation k in bits 2k .. 2k + 1."""
    codes = [OPS.index(n) for n in names]
    if sorted(codes) != [0, 1, 2, 3]:
        raise ValueError("order must be a permutation of %s" % (OPS,))
    return sum(c << (2 * k) for k, c in enumerate(codes))


def empty_params(*shape):
    """A host table of identity records (whole-image boxes are the caller's to fill): no flip, jitter, grayscale, blur, solarise."""
    t = np.zeros(shape, dtype=RECORD_DTYPE)
    t["order"] = pack_order(OPS)
    for k in OPS[:3]:
        t[k] = 1.0
    return t


def _check_tiles(tiles_u8, who):
    if not (isinstance(tiles_u8, torch.Tensor) and tiles_u8.is_cuda and tiles_u8.dtype == torch.uint8 and tiles_u8.dim() == 4
            and tiles_u8.shape[-1] == 3):
        raise _ffi.SnuffyHipError("%s: need a [B, H, W, 3] uint8 GPU tensor (no CPU fallback)" % who)
    ops._on_current_device(tiles_u8, "tiles_u8")
    return tiles_u8.contiguous()


def _check_host_table(t, h, w, size):
    """A table from the host is checked on the host: the kernel clamps what it is given, it does not report."""
    bad = ((t["top"] < 0) | (t["left"] < 0) | (t["ch"] < 1) | (t["cw"] < 1) | (t["top"].astype(np.int64) + t["ch"] > h) |
           (t["left"].astype(np.int64) + t["cw"] > w))
    if bad.any():
        raise _ffi.SnuffyHipError("augment.apply: record %d has a crop box outside the %d x %d tile" % (int(np.argmax(bad)), h, w))
    order = t["order"]
    if any(sorted((int(o) >> (2 * k)) & 3 for k in range(4)) != [0, 1, 2, 3] or int(o) >> 8 for o in np.unique(order)):
        raise _ffi.SnuffyHipError("augment.apply: a record's jitter order is not a permutation of the four operations")
    if not (np.isfinite(t["blur"]).all() and (t["blur"] <= MAX_BLUR_RADIUS).all()):
        raise _ffi.SnuffyHipError("augment.apply: blur radius above %g" % MAX_BLUR_RADIUS)
    for k in OPS:
        if not np.isfinite(t[k]).all():
            raise _ffi.SnuffyHipError("augment.apply: non-finite %s factor" % k)


def draw_params(policies, batch, h, w, sampler):
    """Fills one record per (view, image) on the device from Philox4x32-10 -> int32 [views, batch, 16].  key = the sampler's seed,
    counter = (record index v * batch + i, block, offset); the blocks and their words are listed in DESIGN 4.  The sampler's
    offset moves on by one ON THE DEVICE behind the draw; the host reads nothing back."""
    views, batch = len(policies), int(batch)
    if not (1 <= views <= MAX_VIEWS):
        raise ValueError("draw_params: 1 .. %d views, got %d" % (MAX_VIEWS, views))
    state = sampler.state
    ops._on_current_device(state, "sampler.state")
    rows = [v for p in policies for v in p.row()]
    pol = (ctypes.c_double * len(rows))(*rows)
    params = torch.empty(views, batch, RECORD_WORDS, dtype=torch.int32, device=state.device)
    _ffi.check(_ffi.load().snf_augment_draw(ops._p(state), pol, views, batch, int(h), int(w), ops._p(params), ops._stream()),
               "snf_augment_draw")
    sampler.advance()
    return params


def apply(tiles_u8, params, size):
    """tiles_u8 [B, H, W, 3] uint8 on the GPU, params [R] records with R a multiple of B (record r crops image r % B), either an
    int32 [..., 16] device tensor (as draw_params returns it) or a host RECORD_DTYPE array (checked here, then copied over)
    -> [R, 3, size, size] fp32, (u8 / 255 - mean) / std with the ImageNet constants."""
    tiles_u8 = _check_tiles(tiles_u8, "augment.apply")
    b, h, w, _ = tiles_u8.shape
    size = int(size)
    if isinstance(params, np.ndarray):
        if params.dtype != RECORD_DTYPE:
            raise TypeError("augment.apply: a host table must have dtype augment.RECORD_DTYPE")
        table = np.ascontiguousarray(params).reshape(-1)
        _check_host_table(table, h, w, size)
        params = torch.from_numpy(table.view(np.int32).reshape(-1, RECORD_WORDS)).to(tiles_u8.device)
    if not (isinstance(params, torch.Tensor) and params.is_cuda and params.dtype == torch.int32 and params.shape[-1] == RECORD_WORDS):
        raise _ffi.SnuffyHipError("augment.apply: params must be an int32 [..., %d] GPU tensor or a host RECORD_DTYPE array" % RECORD_WORDS)
    if params.device != tiles_u8.device:
        raise _ffi.SnuffyHipError("augment.apply: params on %s, tiles on %s" % (params.device, tiles_u8.device))
    params = params.contiguous()
    n = params.numel() // RECORD_WORDS
    if n == 0 or n % b:
        raise ValueError("augment.apply: %d records for %d tiles" % (n, b))
    lib = _ffi.load()
    out = torch.empty(n, 3, size, size, dtype=torch.float32, device=tiles_u8.device)
    wsb = lib.snf_augment_workspace_bytes(h, w, size, n)
    ws = ops._ws(wsb, tiles_u8.device)
    mean, std = (ctypes.c_float * 3)(*IMAGENET_MEAN), (ctypes.c_float * 3)(*IMAGENET_STD)
    p = ops._p
    _ffi.check(lib.snf_augment_apply_u8(p(tiles_u8), b, h, w, p(params), n, size, mean, std, p(out), p(ws), wsb, ops._stream()),
               "snf_augment_apply_u8")
    return out


class _Augment:
    def __init__(self, policies, seed):
        self.policies, self.seed, self.sampler = list(policies), seed, None

    def _views(self, tiles_u8, who):
        tiles_u8 = _check_tiles(tiles_u8, who)
        if self.sampler is None:     # seed given: the stream starts at offset 0, so equal seeds draw equal crops
            self.sampler = (ops.DeviceSampler(tiles_u8.device) if self.seed is None else
                            ops.DeviceSampler(tiles_u8.device, seed=self.seed, offset=0))
        b, h, w, _ = tiles_u8.shape
        params = draw_params(self.policies, b, h, w, self.sampler)
        out, v = [], 0
        while v < len(self.policies):            # one launch per run of views of one size
            e = v + 1
            while e < len(self.policies) and self.policies[e].size == self.policies[v].size:
                e += 1
            size = self.policies[v].size
            out += list(apply(tiles_u8, params[v:e], size).view(e - v, b, 3, size, size).unbind(0))
            v = e
        return out


class DINOAugment(_Augment):
    """DataAugmentationDINO on decoded tiles [B, H, W, 3] uint8 on the GPU -> the list of 2 + local_crops_number crop tensors
    ([B, 3, global_size, global_size] x 2, [B, 3, local_size, local_size] x n) that pretrain_dino(augment=...) takes."""

    def __init__(self, global_size=224, local_size=96, local_crops_number=8, global_scale=(0.4, 1.0), local_scale=(0.05, 0.4), seed=None):
        super().__init__(dino_policies(global_size, local_size, local_crops_number, global_scale, local_scale), seed)

    def __call__(self, tiles_u8):
        return self._views(tiles_u8, "DINOAugment")


class MAEAugment(_Augment):
    """The MAE pre-training transform (RandomResizedCrop(size, scale, bicubic) + flip + normalise) on decoded tiles
    [B, H, W, 3] uint8 on the GPU -> [B, 3, size, size] fp32."""

    def __init__(self, size=224, scale=(0.2, 1.0), seed=None):
        super().__init__([mae_policy(size, scale)], seed)

    def __call__(self, tiles_u8):
        return self._views(tiles_u8, "MAEAugment")[0]
