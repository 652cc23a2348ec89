"""Frozen-trunk training route of adapter pre-training (ssl_pretrain.FUSED_TRUNK), the parts that need no GPU: the shape predicate, the
image of W^T the backward GEMMs read, the derivative the backward row kernel restates, and the route stepping aside for CPU tensors."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from snuffy_amd import ops, ssl_pretrain as S, vit

# (m, n, k) of y [m, n] = x [m, k] W [n, k]^T: the trunk's own projections at three widths, rows off every tile grid, and shapes no
# fp32-class form takes (k % 32 != 0, n % 8 != 0, k below the kernels' minimum)
SHAPES = [(34, 192, 64), (34, 64, 256), (111, 384, 128), (12608, 1152, 384), (12608, 384, 1536), (12608, 1536, 384), (44160, 384, 384),
          (12608, 3072, 768), (1, 64, 64), (34, 64, 8), (34, 8, 64), (34, 192, 72), (34, 192, 48), (34, 100, 64), (34, 196, 64),
          (20000, 1156, 384), (64, 64, 16), (34, 4, 64)]


def test_the_predicate_is_image_format_over_a_table():
    seen = set()
    for m, n, k in SHAPES:
        fmt = vit.image_format(m, torch.empty(n, k, device="meta"))
        assert ops.vit_trunk_train_supported(m, n, k) is (fmt is not None), (m, n, k, fmt)
        seen.add(fmt is not None)
    assert seen == {True, False}
    for m, n, k in ((34, 192, 72), (34, 100, 64), (34, 192, 48)):                 # k % 32 != 0 and n % 8 != 0 have no form
        assert not ops.vit_trunk_train_supported(m, n, k)
    assert ops.vit_trunk_train_supported(34, 192, 64) and ops.vit_trunk_train_supported(34, 64, 192)


def test_the_predicate_follows_the_fp32_gemm_setting(monkeypatch):
    monkeypatch.setattr(vit, "FP32_GEMM", "library")
    assert not any(ops.vit_trunk_train_supported(*s) for s in SHAPES)


@pytest.mark.parametrize("fmt", ["hl", "cat"])
def test_the_transposed_image_decodes_to_the_transpose(fmt):
    """hi + lo of the cached W^T image against W.t(): bf16 keeps 8 significant bits, so hi + lo keeps 16 and the rest is below
    2^-17 |w| per element."""
    torch.manual_seed(0)
    lin = torch.nn.Linear(96, 160)
    with torch.no_grad():
        lin.weight.mul_(torch.logspace(-6, 3, 160).unsqueeze(1))
    n, k = lin.weight.shape
    img = S._image_of_t(lin.weight, fmt)
    assert img.dtype == torch.bfloat16 and tuple(img.shape) == (k, (2 if fmt == "hl" else 3) * n)
    if fmt == "hl":
        v = img.view(k, n // 32, 2, 32).float()
        dec = (v[:, :, 0] + v[:, :, 1]).reshape(k, n)
    else:
        assert torch.equal(img[:, :n], img[:, 2 * n:])                           # [Wh | Wl | Wh]
        dec = img[:, :n].float() + img[:, n:2 * n].float()
    wt = lin.weight.detach().t()
    assert bool(((dec - wt).abs() <= 2.0 ** -17 * wt.abs()).all())
    assert S._image_of_t(lin.weight, fmt) is img                                 # cached on the parameter ...
    with torch.no_grad():
        lin.weight.add_(1.0)
    assert S._image_of_t(lin.weight, fmt) is not img                             # ... until it is written again
    assert not hasattr(lin.weight, "_snf_img_" + fmt)                            # under an attribute of its own


def gelu_slope(x):
    """Phi(x) + x phi(x) as csrc/vit_train.hip states it."""
    return 0.5 * (1.0 + torch.erf(x * math.sqrt(0.5))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def test_the_derivative_restated_is_autograd_of_gelu():
    x = torch.cat([torch.linspace(-10, 10, 4001, dtype=torch.float64),
                   torch.tensor([0.0, -0.0, 1e-30, -1e-30, 6.0, -6.0, 40.0, -40.0], dtype=torch.float64)]).requires_grad_(True)
    (g,) = torch.autograd.grad(F.gelu(x).sum(), x)
    ours = gelu_slope(x.detach())
    assert bool(torch.isfinite(ours).all())
    assert float((ours - g).abs().max()) <= 4 * torch.finfo(torch.float64).eps
    assert float(ours[4001]) == 0.5 and float(ours[-2]) == 1.0 and float(ours[-1]) == 0.0


def _frozen_cpu_model():
    model = vit.VisionTransformer(img_size=[32], patch_size=16, embed_dim=64, depth=2, num_heads=1, mlp_ratio=4, qkv_bias=True,
                                  norm_layer=functools.partial(torch.nn.LayerNorm, eps=1e-6), adapter_ffn_layernorm_option="none",
                                  adapter_ffn_init_option="lora", adapter_ffn_scalar="0.1", adapter_ffn_num=8, adapter_d_model=64)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "adaptmlp" in n:
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    for n, p in model.named_parameters():
        p.requires_grad = "adaptmlp" in n
    return model.train()


def test_a_cpu_step_is_bit_identical_with_the_switch_on_and_off(monkeypatch):
    torch.manual_seed(5)
    model = _frozen_cpu_model()
    x = torch.randn(2, 3, 32, 32)
    calls = []
    for name in ("gemm_hl", "gemm_x3", "gelu_image", "gelu_bwd_image"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **kw: calls.append(_n))
    res = {}
    for flag in (True, False):
        monkeypatch.setattr(S, "FUSED_TRUNK", flag)
        model.zero_grad(set_to_none=True)
        torch.manual_seed(7)                                                    # the adapters' dropout draws
        y = S.vit_forward_autograd(model, x)
        y.square().sum().backward()
        res[flag] = [y.detach().clone()] + [p.grad.clone() for p in model.parameters() if p.grad is not None]
    assert len(res[True]) >= 1 + 2 * 4 and not calls
    assert all(torch.equal(a, b) for a, b in zip(res[True], res[False]))
