"""Host side of the ViT self-attention backward above 256 tokens (no GPU): the shape predicates, the routing of ssl_pretrain._attention
away from the kernels on CPU tensors, the float64 yardstick of the GPU suite at its shapes, and the registers of the built kernels."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


def test_long_predicate_is_dk64_above_one_lds_image_up_to_4096():
    from snuffy_amd import ops
    for dk in (32, 64, 128):
        for t in range(0, 4200):
            assert ops.vit_attention_bwd_long_supported(t, dk) is (dk == 64 and 256 < t <= 4096), (t, dk)
    assert ops.VIT_BWD_LONG_MAX_T == 4096


def test_short_predicate_is_unchanged():
    from snuffy_amd import ops
    for dk in (32, 64, 128):
        for t in range(0, 4200):
            assert ops.vit_attention_bwd_supported(t, dk) is (dk == 64 and 1 <= t <= 256), (t, dk)
            assert not (ops.vit_attention_bwd_supported(t, dk) and ops.vit_attention_bwd_long_supported(t, dk))
    assert ops.VIT_BWD_MAX_T == 256


class _Attn(torch.nn.Module):
    def __init__(self, d, h):
        super().__init__()
        self.num_heads, self.scale = h, (d // h) ** -0.5
        self.qkv, self.proj = torch.nn.Linear(d, 3 * d), torch.nn.Linear(d, d)


def _never(*args, **kw):
    raise AssertionError("ViTAttentionFn was entered")


def test_cpu_tensors_take_the_composition_bit_for_bit(monkeypatch):
    from snuffy_amd import ssl_pretrain as S
    torch.manual_seed(0)
    attn = _Attn(128, 2)                                    # dk = 64, T = 300: a shape the long kernels serve on the GPU
    x = torch.randn(1, 300, 128, requires_grad=True)
    monkeypatch.setattr(S.ViTAttentionFn, "apply", _never)
    monkeypatch.setattr(S, "FUSED_ATTENTION", True)
    res = {}
    for flag in (True, False):
        monkeypatch.setattr(S, "FUSED_ATTENTION_LONG", flag)
        x.grad = None
        y = S._attention(attn, x)
        y.square().sum().backward()
        res[flag] = (y.detach().clone(), x.grad.clone())
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])


def test_a_gradient_on_the_gpu_reaches_the_function_only_with_the_switch(monkeypatch):
    """With is_cuda taken out of the question (a tensor subclass that claims the GPU): T = 300 enters ViTAttentionFn with the long switch
    on whatever the short switch says, and takes the composition with it off."""
    from snuffy_amd import ssl_pretrain as S

    class OnGpu(torch.Tensor):
        is_cuda = True

    torch.manual_seed(1)
    attn = _Attn(128, 2)
    entered = []
    monkeypatch.setattr(S.ViTAttentionFn, "apply", lambda qkv, b, t, h, scale: (entered.append((b, t, h)), qkv[:, :qkv.shape[1] // 3])[1])
    x = torch.randn(1, 300, 128).as_subclass(OnGpu).requires_grad_(True)
    for short, long_, expect in ((True, False, []), (False, False, []), (False, True, [(1, 300, 2)]), (True, True, [(1, 300, 2)])):
        monkeypatch.setattr(S, "FUSED_ATTENTION", short)
        monkeypatch.setattr(S, "FUSED_ATTENTION_LONG", long_)
        del entered[:]
        S._attention(attn, x)
        assert entered == expect, (short, long_)


def test_float64_yardstick_is_sane_at_the_gpu_suites_shapes():
    """Every table row of tests/test_gpu_vit_attn_long.py: finite operands and float64 gradients, no zero-norm third."""
    from tests import test_gpu_vit_attn_long as G
    for form in G.FORMS:
        for b, t, h in G.SHAPES:
            qkv, dout, _, lse, dref = G._case(form, b, t, h)
            assert qkv.shape == (b * t, 3 * h * 64) and dout.shape == (b * t, h * 64) and lse.shape == (b, h, t)
            assert bool(torch.isfinite(lse).all()) and dref.dtype == torch.float64
            for name, third in G._thirds(dref):
                assert bool(torch.isfinite(third).all()) and float(third.norm()) > 0, (form, b, t, h, name)


def test_long_kernels_keep_everything_in_registers():
    import scan_spills
    objdir = os.path.join(scan_spills.ROOT, "snuffy_amd", "build")
    if not os.path.isdir(objdir) or not any(f.endswith(".o") for f in os.listdir(objdir)):
        pytest.skip("no build objects here (the library was built elsewhere)")
    try:
        ks = scan_spills.kernels(objdir)
    except RuntimeError as exc:
        pytest.skip(str(exc))
    names = scan_spills.demangle([k[1] for k in ks])
    seen = {"vit_attention_bwd_dq_kernel<": 0, "vit_attention_bwd_dkv_kernel<": 0}
    bad = []
    for (obj, _, scratch, spilled, _vg), name in zip(ks, names):
        for key in seen:
            if key in name:
                seen[key] += 1
                if scratch:
                    bad.append((obj, name[:120], scratch, spilled))
    assert seen == {"vit_attention_bwd_dq_kernel<": 2, "vit_attention_bwd_dkv_kernel<": 2}, seen      # one per arithmetic
    assert not bad, bad
