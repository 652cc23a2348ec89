"""CPU checks of the training augmentations' arithmetic (snuffy_amd/augment.py, csrc/augment.hip): the two host helpers and the
numpy restatement of every stage (tests/augment_ref.py) must equal Pillow bit for bit.  The restatements document what the
kernels compute; Pillow itself is the oracle of the GPU tests (tests/test_gpu_augment.py)."""
import numpy as np
import pytest

from snuffy_amd import augment
from tests import augment_ref as ref

# (h, w) of the crop -> output size
RESIZES = [((150, 200), 224), ((80, 57), 96), ((224, 224), 96), ((23, 31), 224), ((96, 96), 96), ((17, 224), 96), ((3, 5), 32),
           ((1, 1), 32)]
RADII = [0.1, 0.3, 0.77, 1.0, 1.3, 2.0]


def _images(h, w):
    return [ref.noise_image(h, w, seed=h * 1000 + w), ref.smooth_image(h, w)]


@pytest.mark.parametrize("hw,size", RESIZES)
def test_bicubic_coeffs_reproduce_pillow_resize(hw, size):
    h, w = hw
    for img in _images(h, w):
        assert np.array_equal(ref.np_resize(img, (0, 0, h, w), size), ref.pil_resize(img, (0, 0, h, w), size))


def test_bicubic_resize_of_a_box_is_crop_then_resize():
    img = ref.noise_image(64, 80, seed=5)
    box = (7, 11, 40, 33)
    assert np.array_equal(ref.np_resize(img, box, 24), ref.pil_resize(img, box, 24))


def test_bicubic_ksize_stays_inside_the_reserved_row():
    for h, w, s in [(256, 256, 224), (256, 256, 96), (1024, 1024, 128), (40, 56, 24), (96, 80, 32)]:
        for n in (1, 2, s, max(h, w) // 2, max(h, w)):
            bounds, coef, ksize = augment.bicubic_coeffs(n, s)
            assert ksize <= augment.max_ksize(h, w, s) <= 33 and int(bounds[:, 1].max()) <= ksize


@pytest.mark.parametrize("radius", RADII)
def test_gaussian_box_radius_reproduces_pillow_blur(radius):
    for h, w in [(24, 24), (32, 40), (5, 3)]:
        for img in _images(h, w):
            assert np.array_equal(ref.np_blur(img, radius), ref.pil_blur(img, radius)), (radius, h, w)


def test_gaussian_box_radius_on_a_fine_grid():
    img = ref.noise_image(16, 16, seed=3)
    for radius in np.linspace(0.1, 2.0, 77):
        radius = float(np.float32(radius))
        assert np.array_equal(ref.np_blur(img, radius), ref.pil_blur(img, radius)), radius


@pytest.mark.parametrize("name", ["brightness", "contrast", "saturation"])
def test_blend_stages_equal_pillow(name):
    fn = {"brightness": ref.np_brightness, "contrast": ref.np_contrast, "saturation": ref.np_saturation}[name]
    for img in _images(40, 56):
        for f in (0.0, 0.6, 0.8137, 1.0, 1.2, 1.4, float(np.float32(0.9313))):
            assert np.array_equal(fn(img, f), ref.PIL_JITTER[name](img, f)), (name, f)


def test_hue_equals_pillow():
    cube = np.stack(np.meshgrid(np.arange(0, 256, 5), np.arange(0, 256, 5), np.arange(0, 256, 5), indexing="ij"), -1)
    cube = cube.reshape(52, -1, 3).astype(np.uint8)                  # a lattice of the colour cube: every sextant, greys, extremes
    for img in _images(40, 56) + [cube]:
        assert np.array_equal(ref.np_rgb_to_hsv(img), np.asarray(ref.Image.fromarray(img).convert("HSV")))
        for f in (-0.1, -0.05, 0.0, 0.03, 0.1, 0.5, -0.5):
            assert np.array_equal(ref.np_hue(img, f), ref.pil_hue(img, f)), f


def test_luma_grayscale_solarize_equal_pillow():
    for img in _images(40, 56):
        assert np.array_equal(ref.np_luma(img), np.asarray(ref.Image.fromarray(img).convert("L")))
        assert np.array_equal(ref.np_gray(img), ref.pil_gray(img))
        assert np.array_equal(ref.np_solarize(img), ref.pil_solarize(img))


def test_record_layout_and_policies():
    assert augment.RECORD_DTYPE.itemsize == 64
    t = augment.empty_params(3)
    assert ref.record_order(t[0]) == list(augment.OPS)
    assert augment.pack_order(["hue", "brightness", "saturation", "contrast"]) == 3 | (0 << 2) | (2 << 4) | (1 << 6)
    pol = augment.dino_policies()
    assert len(pol) == 10 and [p.size for p in pol] == [224, 224] + [96] * 8
    assert (pol[0].p_blur, pol[0].p_solarize, pol[1].p_blur, pol[1].p_solarize, pol[2].p_blur) == (1.0, 0.0, 0.1, 0.2, 0.5)
    assert all(len(p.row()) == augment.POLICY_WORDS for p in pol)
    mae = augment.mae_policy()
    assert (mae.scale, mae.p_jitter, mae.p_gray, mae.p_blur, mae.p_solarize, mae.p_flip) == ((0.2, 1.0), 0.0, 0.0, 0.0, 0.0, 0.5)


def test_cpu_tensors_are_refused():
    import torch
    from snuffy_amd import SnuffyHipError
    with pytest.raises(SnuffyHipError):
        augment.apply(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), augment.empty_params(1), 8)
    with pytest.raises(SnuffyHipError):
        augment.DINOAugment()(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(SnuffyHipError):
        augment.MAEAugment()(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
