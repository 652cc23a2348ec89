"""The training augmentations on the GPU (snuffy_amd/augment.py, csrc/augment.hip) against Pillow itself, called here on the CPU
with every random decision read from the same parameter record (tests/augment_ref.py: pil_chain).  Every comparison is exact: the
uint8 image recovered from the normalised output equals Pillow's, and the fp32 tensor equals torch's ToTensor + Normalize of it.
The draws are compared with the counter layout restated on the host Philox (oracle/philox_ref.py) and with their distributions."""
import copy
import functools
import itertools
import math

import numpy as np
import pytest
import torch

from snuffy_amd import SnuffyHipError, augment, ops
from tests import augment_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SOURCES = [(40, 56), (96, 80)]
SIZES = [24, 32]
BLEND_FACTORS = [0.6, 1.0, 1.4, 0.0, 0.8137, 1.2]
HUE_FACTORS = [-0.1, 0.0, 0.1, 0.03, -0.05, 0.5]
BLUR_RADII = [0.1, 1.0, 2.0, 0.3, 0.77, 1.3]
ORDERS = list(itertools.permutations(augment.OPS))


@functools.lru_cache(maxsize=None)
def _pair(h, w):
    return [ref.noise_image(h, w, seed=h + w), ref.smooth_image(h, w)]


def _boxes(h, w, size):
    """(top, left, ch, cw): the whole tile, one pixel, a box with ch == cw == size (identity passes), and -- where the tile is large
    enough -- a box reduced 3.5 times (wide antialiasing support)."""
    boxes = [(0, 0, h, w), (h // 2, w // 3, 1, 1), (3, 5, size, size), (2, 1, size, w - 7)]
    big = int(3.5 * size)
    if big <= h:
        boxes.append((h - big, 0, big, min(big, w)))
    return boxes


def _run(imgs, table, size):
    tiles = torch.from_numpy(np.stack(imgs)).to(DEV)
    return augment.apply(tiles, table, size).cpu().numpy()


def _check(out, imgs, table, size):
    flat = table.reshape(-1)
    assert out.shape == (flat.size, 3, size, size)
    for r in range(flat.size):
        want = ref.pil_chain(imgs[r % len(imgs)], flat[r], size)
        got = ref.recover_u8(out[r])
        bad = int((got != want).sum())
        assert bad == 0, "record %d %r: %d of %d bytes differ from Pillow" % (r, flat[r], bad, want.size)
        assert np.array_equal(out[r], ref.to_tensor_normalize(want)), "record %d: fp32 differs from ToTensor + Normalize" % r


def _stage_records(stage, box):
    """The records that run `stage` alone on `box` (the other jitter factors neutral; a jitter always makes the HSV round trip)."""
    base = augment.empty_params(1)[0]
    base["top"], base["left"], base["ch"], base["cw"] = box
    recs = []

    def variant(**kw):
        r = base.copy()
        for k, v in kw.items():
            r[k] = v
        recs.append(r)

    if stage == "resize":
        variant()
    elif stage == "flip":
        variant(flip=1)
    elif stage in ("brightness", "contrast", "saturation"):
        for f in BLEND_FACTORS:
            variant(jitter=1, order=augment.pack_order([stage] + [o for o in augment.OPS if o != stage]), **{stage: f})
    elif stage == "hue":
        for f in HUE_FACTORS:
            variant(jitter=1, hue=f)
    elif stage == "gray":
        variant(gray=1)
    elif stage == "blur":
        for radius in BLUR_RADII:
            variant(blur=radius)
    elif stage == "solarize":
        variant(solarize=1)
    return recs


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("hw", SOURCES)
@pytest.mark.parametrize("stage", ["resize", "flip", "brightness", "contrast", "saturation", "hue", "gray", "blur", "solarize"])
def test_one_stage_equals_pillow(stage, hw, size):
    imgs = _pair(*hw)
    recs = [r for box in _boxes(hw[0], hw[1], size) for r in _stage_records(stage, box) for _ in imgs]   # record r crops image r % 2
    table = np.array(recs, dtype=augment.RECORD_DTYPE)
    _check(_run(imgs, table, size), imgs, table, size)


def _composed_table(n_img, h, w, seed):
    """3 views x n_img images: all 24 jitter orders, with and without every optional stage, boxes of every proportion."""
    rng = np.random.default_rng(seed)
    t = augment.empty_params(3, n_img)
    for k, rec in enumerate(t.reshape(-1)):
        ch, cw = int(rng.integers(1, h + 1)), int(rng.integers(1, w + 1))
        rec["top"], rec["left"], rec["ch"], rec["cw"] = int(rng.integers(0, h - ch + 1)), int(rng.integers(0, w - cw + 1)), ch, cw
        rec["flip"], rec["jitter"], rec["gray"], rec["solarize"] = k & 1, k % 25 != 24, (k >> 1) & 1, (k >> 2) & 1
        rec["order"] = augment.pack_order(ORDERS[k % 24])
        rec["brightness"], rec["contrast"], rec["saturation"] = rng.uniform(0.6, 1.4), rng.uniform(0.6, 1.4), rng.uniform(0.8, 1.2)
        rec["hue"] = rng.uniform(-0.1, 0.1)
        rec["blur"] = rng.uniform(0.1, 2.0) if k % 3 else 0.0
    return t


def test_composed_chain_equals_pillow():
    h, w, size = 64, 72, 32
    imgs = [ref.noise_image(h, w, seed=i) if i % 2 else np.roll(ref.smooth_image(h, w), 7 * i, axis=1) for i in range(8)]
    table = _composed_table(8, h, w, seed=11)
    flat = table.reshape(-1)
    assert len({int(o) for o in flat["order"][flat["jitter"] != 0]}) == 24
    for name in ("flip", "gray", "solarize"):
        assert 0 < int((flat[name] != 0).sum()) < flat.size
    assert 0 < int((flat["blur"] > 0).sum()) < flat.size
    _check(_run(imgs, table, size), imgs, table, size)


@pytest.mark.parametrize("size", [224, 96])
def test_recipe_sizes_equal_pillow(size):
    imgs = [ref.noise_image(256, 256, seed=1), ref.smooth_image(256, 256)]
    table = augment.empty_params(2, 2)
    boxes = {224: [(10, 20, 200, 230), (0, 0, 256, 256), (31, 5, 224, 171), (100, 90, 130, 150)],
             96: [(0, 0, 256, 256), (60, 70, 57, 80), (128, 100, 96, 110), (7, 9, 240, 200)]}[size]
    for k, rec in enumerate(table.reshape(-1)):
        rec["top"], rec["left"], rec["ch"], rec["cw"] = boxes[k]
        rec["flip"], rec["jitter"], rec["gray"], rec["solarize"] = k & 1, 1, k == 3, k >= 2
        rec["order"] = augment.pack_order(ORDERS[(7 * k + 3) % 24])
        rec["brightness"], rec["contrast"], rec["saturation"], rec["hue"] = 0.7 + 0.2 * k, 1.35 - 0.2 * k, 0.85 + 0.1 * k, 0.09 - 0.05 * k
        rec["blur"] = [1.7, 0.0, 0.4, 2.0][k]
    _check(_run(imgs, table, size), imgs, table, size)


def test_output_is_independent_of_batch_position_and_size():
    h, w, size = 40, 56, 24
    x = ref.smooth_image(h, w)
    rows = _composed_table(1, h, w, seed=5)[:, 0]                  # three records for x
    alone = _run([x], rows, size)
    for b, pos in ((3, 1), (130, 77)):
        imgs = [ref.noise_image(h, w, seed=100 + i) for i in range(b)]
        imgs[pos] = x
        table = _composed_table(b, h, w, seed=b)                   # 3 b records: 390 > two workgroups per CU would need 512 ...
        table = np.concatenate([table, table[:1]])                 # ... so a fourth view: 520 records walk the grid twice
        table[:3, pos] = rows
        table[3, pos] = rows[0]
        out = _run(imgs, table, size)
        assert np.array_equal(out, _run(imgs, table, size))        # repeat calls are bit-identical
        out = out.reshape(4, b, 3, size, size)
        assert np.array_equal(out[:3, pos], alone) and np.array_equal(out[3, pos], alone[0])
        if b == 130:
            _check(out.reshape(-1, 3, size, size), imgs, table, size)


def _device_draw(policies, batch, h, w, seed, offset):
    sampler = ops.DeviceSampler(DEV, seed=seed, offset=offset)
    params = augment.draw_params(policies, batch, h, w, sampler)
    assert params.shape == (len(policies), batch, augment.RECORD_WORDS) and params.dtype == torch.int32
    assert sampler.state.cpu().tolist() == [seed, offset + 1]      # the offset moved on, on the device
    return params.cpu().numpy().view(augment.RECORD_DTYPE).reshape(len(policies), batch)


def test_draws_reproduce_on_the_host():
    policies = augment.dino_policies()
    seed, offset = 0x1234567890ABCDE, (5 << 32) + 17
    for h, w in ((256, 256), (64, 256)):
        dev = _device_draw(policies, 64, h, w, seed, offset)
        host, raw = ref.host_draw(policies, 64, h, w, seed, offset)
        for name in ("flip", "jitter", "order", "gray", "solarize", "fallback", "brightness", "contrast", "saturation", "hue", "blur"):
            assert np.array_equal(dev[name], host[name]), name
        # the sides go through exp and sqrt: +-1 only where the unrounded side is within 1e-9 of a half-integer
        same = np.ones(dev.shape, dtype=bool)
        for i, name in enumerate(("ch", "cw")):
            diff = dev[name].astype(np.int64) - host[name]
            near_half = np.abs(np.abs(raw[..., i] - np.floor(raw[..., i])) - 0.5) < 1e-9
            assert np.all((diff == 0) | ((np.abs(diff) == 1) & near_half)), name
            same &= diff == 0
        assert same.mean() > 0.99
        for name in ("top", "left"):
            assert np.array_equal(dev[name][same], host[name][same]), name
    assert not np.array_equal(_device_draw(policies, 64, 256, 256, seed, offset + 1)["top"], dev["top"])


def _within(count, n, p, what):
    sigma = math.sqrt(n * p * (1.0 - p))
    assert abs(count - n * p) <= 5.0 * sigma, "%s: %d of %d at p = %g (5 sigma = %.1f)" % (what, count, n, p, 5.0 * sigma)


def test_draw_statistics():
    policies = augment.dino_policies()
    b, h, w = 4096, 256, 256
    t = _device_draw(policies, b, h, w, seed=20261021, offset=3)
    groups = {"global 1": t[0:1], "global 2": t[1:2], "local": t[2:]}
    for name, g in groups.items():
        pol = policies[{"global 1": 0, "global 2": 1, "local": 2}[name]]
        n = g.size
        _within(int((g["flip"] != 0).sum()), n, pol.p_flip, name + " flip")
        _within(int((g["jitter"] != 0).sum()), n, pol.p_jitter, name + " jitter")
        _within(int((g["gray"] != 0).sum()), n, pol.p_gray, name + " grayscale")
        _within(int((g["blur"] > 0).sum()), n, pol.p_blur, name + " blur")              # p = 0 or 1: sigma = 0, the count is exact
        _within(int((g["solarize"] != 0).sum()), n, pol.p_solarize, name + " solarise")
        radii = g["blur"][g["blur"] > 0]
        assert radii.min() >= np.float32(0.1) and radii.max() <= np.float32(2.0)
        assert abs(radii.mean() - 1.05) <= 5.0 * (1.9 / math.sqrt(12.0)) / math.sqrt(radii.size)
        frac = g["ch"].astype(np.float64) * g["cw"] / (h * w)
        assert frac.min() >= pol.scale[0] * 0.97 - 2.0 / h and frac.max() <= pol.scale[1] * 1.03 + 2.0 / h
    flat = t.reshape(-1)
    n = flat.size
    counts = {int(o): int(c) for o, c in zip(*np.unique(flat["order"], return_counts=True))}
    assert sorted(counts) == sorted(augment.pack_order(o) for o in ORDERS)
    for o, c in counts.items():
        _within(c, n, 1.0 / 24.0, "order %d" % o)
    for name, half in zip(augment.OPS, policies[0].jitter):
        centre = 0.0 if name == "hue" else 1.0
        f = flat[name]
        assert f.min() >= np.float32(centre - half) and f.max() <= np.float32(centre + half), name
        assert abs(f.mean(dtype=np.float64) - centre) <= 5.0 * (2.0 * half / math.sqrt(12.0)) / math.sqrt(n), name
    for g in (flat,):
        assert (g["ch"] >= 1).all() and (g["cw"] >= 1).all() and (g["top"] >= 0).all() and (g["left"] >= 0).all()
        assert (g["top"] + g["ch"] <= h).all() and (g["left"] + g["cw"] <= w).all()
    assert int(flat["fallback"].sum()) == 0                                              # a square tile always accepts a try
    # a 4 : 1 tile: no global try fits its height, so the centred crop (full height, aspect clamped to 4 / 3) is taken
    t = _device_draw(policies, 64, 64, 256, seed=7, offset=0)
    fb = t[t["fallback"] != 0]
    assert fb.size >= 128 and (t[:2]["fallback"] != 0).all()
    assert (fb["ch"] == 64).all() and (fb["cw"] == 85).all() and (fb["top"] == 0).all() and (fb["left"] == (256 - 85) // 2).all()
    ok = t[t["fallback"] == 0]
    assert (ok["top"] + ok["ch"] <= 64).all() and (ok["left"] + ok["cw"] <= 256).all() and (ok["ch"] >= 1).all() and (ok["cw"] >= 1).all()


def _tiles(b, h=256, w=256):
    return torch.from_numpy(np.stack([ref.noise_image(h, w, seed=i) if i % 2 else np.roll(ref.smooth_image(h, w), 31 * i, axis=0)
                                      for i in range(b)])).to(DEV)


def test_dino_augment_feeds_a_training_step():
    from snuffy_amd import ssl_pretrain as S
    from tests import test_ssl_pretrain as T
    tiles = _tiles(4)
    aug = augment.DINOAugment(seed=5)
    crops = aug(tiles)
    assert [tuple(c.shape) for c in crops] == [(4, 3, 224, 224)] * 2 + [(4, 3, 96, 96)] * 8
    assert all(c.dtype == torch.float32 and bool(torch.isfinite(c).all()) for c in crops)
    again = augment.DINOAugment(seed=5)(tiles)
    other = augment.DINOAugment(seed=6)(tiles)
    assert all(torch.equal(a, c) for a, c in zip(again, crops))
    assert not any(torch.equal(a, c) for a, c in zip(other, crops))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")          # the second call of a warm object: no device -> host copy, no synchronisation
    try:
        second = aug(tiles)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert not torch.equal(second[0], crops[0])      # the offset advanced on the device
    torch.manual_seed(0)
    student, teacher = T._student().to(DEV).train(), T._student().to(DEV).train()
    teacher.load_state_dict(student.state_dict())
    for p in teacher.parameters():
        p.requires_grad = False
    S.freeze_for_adapter_tuning(student)
    opt = torch.optim.AdamW(S.get_params_groups(student), lr=1e-3, weight_decay=0.04)
    loss = S.dino_train_step(student, teacher, S.DINOLoss(48, 10, 0.04, 0.07, 3, 10).to(DEV), crops, opt, epoch=1, it=0,
                             momentum_schedule=np.array([0.99]), clip_grad=0.3, freeze_last_layer=1)
    assert math.isfinite(float(loss))


def test_mae_augment_in_the_pretraining_loop():
    from snuffy_amd import ssl_pretrain as S
    from tests import test_ssl_pretrain as T
    tiles = _tiles(4, 80, 96)
    aug = augment.MAEAugment(size=64, seed=9)
    imgs = aug(tiles)
    assert tuple(imgs.shape) == (4, 3, 64, 64) and bool(torch.isfinite(imgs).all())
    torch.manual_seed(1)
    model = T._mae().to(DEV)
    losses = S.pretrain_mae(copy.deepcopy(model), lambda e: iter([tiles]), epochs=1, niter_per_ep=1, augment=aug)
    assert len(losses) == 1 and math.isfinite(losses[0])
    # augment = None is the call as it was: the same loss, bit for bit
    floats = torch.rand(4, 3, 64, 64, device=DEV)
    got = []
    for kw in ({}, {"augment": None}):
        torch.manual_seed(2)
        got.append(S.pretrain_mae(copy.deepcopy(model), lambda e: iter([floats]), epochs=1, niter_per_ep=1, **kw))
    assert got[0] == got[1] and math.isfinite(got[0][0])


def test_refusals():
    table = augment.empty_params(1)
    table["ch"], table["cw"] = 40, 56
    good = torch.zeros(1, 40, 56, 3, dtype=torch.uint8, device=DEV)
    assert augment.apply(good, table, 24).shape == (1, 3, 24, 24)
    with pytest.raises(SnuffyHipError):
        augment.apply(good.cpu(), table, 24)                                               # no CPU fallback
    with pytest.raises(SnuffyHipError):
        augment.apply(good.float(), table, 24)                                             # decoded tiles are uint8
    with pytest.raises(SnuffyHipError):
        augment.DINOAugment()(good.float())
    with pytest.raises(SnuffyHipError, match=r"code -3"):
        augment.apply(good, table, augment.MAX_SIZE + 1)                                   # size outside the kernel
    with pytest.raises(SnuffyHipError, match=r"code -3"):
        augment.apply(good, table, 6)                                                      # 56 > 8 * 6: a reduction above 8
    for field, value in (("top", 1), ("left", -1), ("cw", 57), ("ch", 0)):
        bad = table.copy()
        bad[field] = value
        with pytest.raises(SnuffyHipError, match="outside"):
            augment.apply(good, bad, 24)                                                   # checked on the host, before any launch
    with pytest.raises(SnuffyHipError):
        augment.apply(good, torch.from_numpy(table.view(np.int32).reshape(1, 16)), 24)     # a device table must be on the device
