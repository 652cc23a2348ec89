"""Host side of the differentiable ViT self-attention (no GPU): the shape predicate, the routing of ssl_pretrain._attention away from
the kernels, and the registers of the built kernels."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


def test_bwd_supported_is_dk64_and_one_lds_image_of_keys():
    from snuffy_amd import ops
    for dk in (32, 64, 128):
        for t in range(0, 301):
            assert ops.vit_attention_bwd_supported(t, dk) is (dk == 64 and 1 <= t <= 256), (t, dk)
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
    attn = _Attn(128, 2)                                    # dk = 64, T = 37: a shape the kernels serve on the GPU
    x = torch.randn(2, 37, 128, requires_grad=True)
    monkeypatch.setattr(S.ViTAttentionFn, "apply", _never)
    res = {}
    for flag in (True, False):
        monkeypatch.setattr(S, "FUSED_ATTENTION", flag)
        x.grad = None
        y = S._attention(attn, x)
        y.square().sum().backward()
        res[flag] = (y.detach().clone(), x.grad.clone())
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])


def test_no_gradient_asked_for_means_no_autograd_function(monkeypatch):
    """The condition is on qkv.requires_grad: with is_cuda taken out of the question (a tensor subclass that claims the GPU), a frozen
    input through frozen weights still takes the composition, and the same call with a gradient asked for reaches the function."""
    from snuffy_amd import ssl_pretrain as S

    class OnGpu(torch.Tensor):
        is_cuda = True

        @classmethod
        def __torch_function__(cls, func, types, args=(), kwargs=None):
            out = super().__torch_function__(func, types, args, kwargs or {})
            return out

    torch.manual_seed(1)
    attn = _Attn(128, 2)
    for p in attn.parameters():
        p.requires_grad = False
    entered = []
    monkeypatch.setattr(S, "FUSED_ATTENTION", True)
    monkeypatch.setattr(S.ViTAttentionFn, "apply", lambda qkv, b, t, h, scale: (entered.append((b, t, h)), qkv[:, :qkv.shape[1] // 3])[1])
    x = torch.randn(2, 37, 128).as_subclass(OnGpu)
    S._attention(attn, x)
    assert not entered
    S._attention(attn, x.clone().requires_grad_(True))
    assert entered == [(2, 37, 2)]


def test_new_kernels_keep_everything_in_registers():
    import scan_spills
    objdir = os.path.join(scan_spills.ROOT, "snuffy_amd", "build")
    if not os.path.isdir(objdir) or not any(f.endswith(".o") for f in os.listdir(objdir)):
        pytest.skip("no build objects here (the library was built elsewhere)")
    try:
        ks = scan_spills.kernels(objdir)
    except RuntimeError as exc:
        pytest.skip(str(exc))
    names = scan_spills.demangle([k[1] for k in ks])
    seen = {"vit_attention_bwd_kernel<": 0, "vit_attention_bwd_t1_kernel<": 0, "vit_attention_mfma_kernel<": 0}
    bad = []
    for (obj, _, scratch, spilled, _vg), name in zip(ks, names):
        for key in seen:
            if key in name:
                seen[key] += 1
                if scratch:
                    bad.append((obj, name[:120], scratch, spilled))
    # backward: 4 key-block counts x 2 arithmetics; forward (the lse store is a nullable pointer of the same instantiations): 5 + 4
    assert seen == {"vit_attention_bwd_kernel<": 8, "vit_attention_bwd_t1_kernel<": 2, "vit_attention_mfma_kernel<": 9}, seen
    assert not bad, bad
