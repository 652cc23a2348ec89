"""Shared by the augmentation tests: the reference's per-crop chain written with Pillow calls (the oracle), and numpy restatements
of each stage's arithmetic as DESIGN 4 documents it (what csrc/augment.hip computes; tests/test_augment_host.py pins each one
to Pillow wherever the suite runs).  An image is an [h, w, 3] uint8 array; a record is one element of augment.RECORD_DTYPE."""
import numpy as np
from PIL import Image, ImageEnhance, ImageFilter, ImageOps

from snuffy_amd import augment

MEAN = np.array(augment.IMAGENET_MEAN, dtype=np.float32)
STD = np.array(augment.IMAGENET_STD, dtype=np.float32)
F32 = np.float32


# ---- Pillow: the oracle -------------------------------------------------------------------------------------------------------
def pil_resize(img, box, size):
    """box = (top, left, ch, cw)"""
    top, left, ch, cw = box
    return np.asarray(Image.fromarray(img).crop((left, top, left + cw, top + ch)).resize((size, size), Image.BICUBIC))


def pil_flip(img):
    return np.asarray(Image.fromarray(img).transpose(Image.FLIP_LEFT_RIGHT))


def pil_brightness(img, f):
    return np.asarray(ImageEnhance.Brightness(Image.fromarray(img)).enhance(f))


def pil_contrast(img, f):
    return np.asarray(ImageEnhance.Contrast(Image.fromarray(img)).enhance(f))


def pil_saturation(img, f):
    return np.asarray(ImageEnhance.Color(Image.fromarray(img)).enhance(f))


def pil_hue(img, f):
    h, s, v = Image.fromarray(img).convert("HSV").split()
    nh = ((np.asarray(h).astype(np.int64) + int(f * 255)) % 256).astype(np.uint8)
    return np.asarray(Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB"))


def pil_gray(img):
    l = Image.fromarray(img).convert("L")
    return np.asarray(Image.merge("RGB", (l, l, l)))


def pil_blur(img, radius):
    return np.asarray(Image.fromarray(img).filter(ImageFilter.GaussianBlur(radius=radius)))


def pil_solarize(img):
    return np.asarray(ImageOps.solarize(Image.fromarray(img), 128))


PIL_JITTER = {"brightness": pil_brightness, "contrast": pil_contrast, "saturation": pil_saturation, "hue": pil_hue}


def record_order(rec):
    return [augment.OPS[(int(rec["order"]) >> (2 * k)) & 3] for k in range(4)]


def pil_chain(img, rec, size):
    """The reference's transform with every random decision read from the record -> the final uint8 image [size, size, 3]."""
    x = pil_resize(img, (int(rec["top"]), int(rec["left"]), int(rec["ch"]), int(rec["cw"])), size)
    if rec["flip"]:
        x = pil_flip(x)
    if rec["jitter"]:
        for name in record_order(rec):
            x = PIL_JITTER[name](x, float(rec[name]))
    if rec["gray"]:
        x = pil_gray(x)
    if rec["blur"] > 0:
        x = pil_blur(x, float(rec["blur"]))
    if rec["solarize"]:
        x = pil_solarize(x)
    return x


def to_tensor_normalize(u8):
    """torch's ToTensor + Normalize on an [.., s, s, 3] uint8 image -> [.., 3, s, s] fp32, in fp32 on the CPU."""
    import torch
    t = torch.from_numpy(np.array(u8)).movedim(-1, -3).to(torch.float32) / 255.0
    return ((t - torch.tensor(MEAN).view(3, 1, 1)) / torch.tensor(STD).view(3, 1, 1)).numpy()


def recover_u8(out):
    """The uint8 image behind a normalised fp32 crop [.., 3, s, s] -> [.., s, s, 3]."""
    v = np.rint((out.astype(np.float64) * STD.reshape(3, 1, 1) + MEAN.reshape(3, 1, 1)) * 255.0)
    return np.moveaxis(v, -3, -1).astype(np.uint8)


# ---- numpy restatements -------------------------------------------------------------------------------------------------------
def _resample_axis0(img, n_out):
    bounds, coef, _ = augment.bicubic_coeffs(img.shape[0], n_out)
    out = np.empty((n_out,) + img.shape[1:], dtype=np.uint8)
    src = img.astype(np.int64)
    for o in range(n_out):
        lo, cnt = bounds[o]
        ss = (1 << (augment.PRECISION_BITS - 1)) + np.tensordot(coef[o, :cnt].astype(np.int64), src[lo:lo + cnt], axes=(0, 0))
        out[o] = np.clip(ss >> augment.PRECISION_BITS, 0, 255)
    return out


def np_resize(img, box, size):
    top, left, ch, cw = box
    crop = img[top:top + ch, left:left + cw]
    horiz = _resample_axis0(crop.transpose(1, 0, 2), size).transpose(1, 0, 2)      # horizontal pass first, uint8 between the passes
    return _resample_axis0(horiz, size)


def np_luma(img):
    r, g, b = (img[..., c].astype(np.int64) for c in range(3))
    return ((19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16).astype(np.uint8)


def np_blend(deg, img, f):
    """deg + f * (img - deg) in float32, multiply and add rounded separately"""
    f = F32(f)
    deg = np.broadcast_to(np.asarray(deg), img.shape).astype(F32)
    t = (deg + (f * (img.astype(F32) - deg)).astype(F32)).astype(F32)
    if 0.0 <= f <= 1.0:
        return t.astype(np.uint8)
    return np.clip(t, 0, 255).astype(np.uint8)


def np_brightness(img, f):
    return np_blend(0, img, f)


def np_contrast(img, f):
    l = np_luma(img).astype(np.int64)
    return np_blend((2 * int(l.sum()) + l.size) // (2 * l.size), img, f)


def np_saturation(img, f):
    return np_blend(np_luma(img)[..., None], img, f)


def np_gray(img):
    return np.repeat(np_luma(img)[..., None], 3, axis=-1)


def np_rgb_to_hsv(img):
    r, g, b = (img[..., c].astype(np.int64) for c in range(3))
    maxc, minc = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    grey = maxc == minc
    with np.errstate(divide="ignore", invalid="ignore"):
        cr = (maxc - minc).astype(F32)
        s = cr / maxc.astype(F32)
        rc, gc, bc = ((maxc - c).astype(F32) / cr for c in (r, g, b))
        h = np.where(r == maxc, bc - gc,
                     np.where(g == maxc, (2.0 + rc.astype(np.float64) - bc.astype(np.float64)).astype(F32),
                              (4.0 + gc.astype(np.float64) - rc.astype(np.float64)).astype(F32))).astype(F32)
        h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(F32)
        uh = np.clip(np.nan_to_num(h.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
        us = np.clip(np.nan_to_num(s.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
    return np.stack([np.where(grey, 0, uh), np.where(grey, 0, us), maxc], axis=-1).astype(np.uint8)


def _round_half_away(x):
    return np.clip(np.floor(x.astype(np.float64) + 0.5), 0, 255).astype(np.uint8)


def np_hsv_to_rgb(hsv):
    hh, ss, v = hsv[..., 0], hsv[..., 1], hsv[..., 2]
    h = (hh.astype(F32) * F32(6.0)) / F32(255.0)
    i = np.floor(h)
    f = (h - i).astype(F32)
    fs = ss.astype(F32) / F32(255.0)
    one, vf = F32(1.0), v.astype(F32)
    p = _round_half_away(vf * (one - fs))
    q = _round_half_away(vf * (one - fs * f))
    t = _round_half_away(vf * (one - fs * (one - f)))
    sext = i.astype(np.int64) % 6
    table = [(v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q)]
    out = np.stack([np.choose(sext, [row[c] for row in table]) for c in range(3)], axis=-1)
    return np.where((ss == 0)[..., None], v[..., None], out).astype(np.uint8)


def np_hue(img, f):
    hsv = np_rgb_to_hsv(img)
    hsv[..., 0] = (hsv[..., 0].astype(np.int64) + int(float(F32(f)) * 255)) % 256
    return np_hsv_to_rgb(hsv)


def _box_pass_axis1(img, r, ww, fw):
    n = img.shape[1]
    src = img.astype(np.int64)
    idx = np.arange(n)
    bulk = np.zeros_like(src)
    for d in range(-r, r + 1):
        bulk += src[:, np.clip(idx + d, 0, n - 1)]
    edge = src[:, np.clip(idx - r - 1, 0, n - 1)] + src[:, np.clip(idx + r + 1, 0, n - 1)]
    return ((bulk * ww + edge * fw + (1 << 23)) >> 24).astype(np.uint8)


def np_blur(img, radius):
    big_r, ww, fw = augment.gaussian_box_radius(radius)
    x = img
    for _ in range(3):
        x = _box_pass_axis1(x, int(big_r), ww, fw)
    x = x.transpose(1, 0, 2)
    for _ in range(3):
        x = _box_pass_axis1(x, int(big_r), ww, fw)
    return x.transpose(1, 0, 2)


def np_solarize(img):
    return np.where(img < 128, img, 255 - img).astype(np.uint8)


# ---- the draws: the counter layout of snf_augment_draw on the host Philox -------------------------------------------------------
def host_draw(policies, batch, h, w, seed, offset):
    """-> (records [views, batch] RECORD_DTYPE, raw [views, batch, 2] = the unrounded (ch, cw) of the accepted try, NaN for a
    centred fallback).  key = seed, counter = (record v * batch + i, block, offset); u = (x + 1/2) / 2^32; integers floor(x n / 2^32);
    Bernoulli x < p 2^32."""
    import itertools

    from oracle.philox_ref import philox4x32_10
    views = len(policies)
    n = views * batch
    r = np.arange(n, dtype=np.uint64)
    pol = np.array([p.row() for p in policies], dtype=np.float64)[np.arange(n) // batch]
    mask = 0xFFFFFFFF

    def block(j):
        return philox4x32_10(r, np.full(n, j, dtype=np.uint64), np.full(n, offset & mask, dtype=np.uint64),
                             np.full(n, (offset >> 32) & mask, dtype=np.uint64), seed & mask, (seed >> 32) & mask)

    def unit(x):
        return (x.astype(np.float64) + 0.5) / 4294967296.0

    def below(x, m):
        return ((x * m.astype(np.uint64)) >> np.uint64(32)).astype(np.int64)

    def between(x, lo, hi):
        return (lo + (hi - lo) * unit(x)).astype(np.float32)

    def bernoulli(x, p):
        return x.astype(np.float64) < p * 4294967296.0

    rec = np.zeros(n, dtype=augment.RECORD_DTYPE)
    raw = np.full((n, 2), np.nan)
    have = np.zeros(n, dtype=bool)
    for t in range(augment.DRAW_TRIES):
        x = block(t)
        area = (pol[:, 0] + (pol[:, 1] - pol[:, 0]) * unit(x[0])) * (float(h) * float(w))
        ratio = np.exp(augment.LOG_RATIO_LO + (augment.LOG_RATIO_HI - augment.LOG_RATIO_LO) * unit(x[1]))
        cw_raw, ch_raw = np.sqrt(area * ratio), np.sqrt(area / ratio)
        cw, ch = np.rint(cw_raw), np.rint(ch_raw)
        take = ~have & (cw > 0) & (cw <= w) & (ch > 0) & (ch <= h)
        chi, cwi = np.where(take, ch, 1).astype(np.int64), np.where(take, cw, 1).astype(np.int64)
        for name, val in (("ch", chi), ("cw", cwi), ("top", below(x[2], h - chi + 1)), ("left", below(x[3], w - cwi + 1))):
            rec[name][take] = val[take]
        raw[take, 0], raw[take, 1] = ch_raw[take], cw_raw[take]
        have |= take
    fb_h, fb_w = h, w
    if w / h < 0.75:
        fb_h = int(np.rint(w / 0.75))
    elif w / h > 4.0 / 3.0:
        fb_w = int(np.rint(h * (4.0 / 3.0)))
    fb_h, fb_w = min(max(fb_h, 1), h), min(max(fb_w, 1), w)
    for name, val in (("ch", fb_h), ("cw", fb_w), ("top", (h - fb_h) // 2), ("left", (w - fb_w) // 2), ("fallback", 1)):
        rec[name][~have] = val
    x = block(augment.BLOCK_FLAGS)
    rec["flip"], rec["jitter"], rec["gray"] = bernoulli(x[0], pol[:, 2]), bernoulli(x[1], pol[:, 3]), bernoulli(x[2], pol[:, 12])
    blur = bernoulli(x[3], pol[:, 13])
    x = block(augment.BLOCK_MISC)
    rec["solarize"] = bernoulli(x[0], pol[:, 16])
    rec["blur"] = np.where(blur, between(x[1], pol[:, 14], pol[:, 15]), np.float32(0))
    perms = np.array([sum(c << (2 * i) for i, c in enumerate(p)) for p in itertools.permutations(range(4))])
    rec["order"] = perms[below(x[2], np.full(n, 24))]
    x = block(augment.BLOCK_FACTORS)
    for i, name in enumerate(augment.OPS):
        rec[name] = between(x[i], pol[:, 4 + 2 * i], pol[:, 5 + 2 * i])
    return rec.reshape(views, batch), raw.reshape(views, batch, 2)


# ---- test images --------------------------------------------------------------------------------------------------------------
def noise_image(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def smooth_image(h, w):
    """Smooth gradients with a saturated red, a saturated blue, a white, a black and a mid-grey region."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([127.5 + 127.5 * np.sin(x / 7.0 + y / 11.0), 255.0 * x / max(w - 1, 1), 255.0 * (1.0 - y / max(h - 1, 1))], axis=-1)
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    qh, qw = max(h // 4, 1), max(w // 4, 1)
    img[:qh, :qw] = (255, 0, 0)
    img[:qh, -qw:] = (0, 0, 255)
    img[-qh:, :qw] = 255
    img[-qh:, -qw:] = 0
    img[h // 2 - qh // 2:h // 2 + qh // 2 + 1, w // 2 - qw // 2:w // 2 + qw // 2 + 1] = 128
    return img
