"""Host side of the 32-wide differentiable ViT self-attention (csrc/vit_attn_dk32.hip; no GPU): the shape predicates, the routing of
ssl_pretrain._attention at dk = 32, and the registers of the built kernels."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

NKB_BUILT = (2, 4, 8)       # key-block counts the dispatch of csrc/vit_attn_dk32.hip builds, each in two arithmetics


def test_predicate_table_and_the_older_predicates_unchanged():
    from snuffy_amd import ops
    assert ops.VIT_DK32_MAX_T == 256
    for dk in (16, 32, 64, 128):
        for t in range(0, 301):
            assert ops.vit_attention_dk32_supported(t, dk) is (dk == 32 and 1 <= t <= 256), (t, dk)
            assert ops.vit_attention_bwd_supported(t, dk) is (dk == 64 and 1 <= t <= 256), (t, dk)
            assert ops.vit_attention_bwd_long_supported(t, dk) is (dk == 64 and t > 256), (t, dk)
    for dk in (16, 32, 64, 128):
        for t in (257, 785, 4096, 4097):
            assert ops.vit_attention_bwd_long_supported(t, dk) is (dk == 64 and t <= 4096), (t, dk)
            assert ops.vit_attention_dk32_supported(t, dk) is False


class _Attn(torch.nn.Module):
    def __init__(self, d, h):
        super().__init__()
        self.num_heads, self.scale = h, (d // h) ** -0.5
        self.qkv, self.proj = torch.nn.Linear(d, 3 * d), torch.nn.Linear(d, d)


def _never(*args, **kw):
    raise AssertionError("ViTAttentionFn was entered")


def test_cpu_tensors_at_dk32_take_the_composition_bit_for_bit(monkeypatch):
    from snuffy_amd import ssl_pretrain as S
    torch.manual_seed(0)
    attn = _Attn(64, 2)                                     # dk = 32, T = 37: a shape the kernels serve on the GPU
    x = torch.randn(2, 37, 64, requires_grad=True)
    monkeypatch.setattr(S.ViTAttentionFn, "apply", _never)
    res = {}
    for flag in (True, False):
        monkeypatch.setattr(S, "FUSED_ATTENTION_DK32", flag)
        x.grad = None
        y = S._attention(attn, x)
        y.square().sum().backward()
        res[flag] = (y.detach().clone(), x.grad.clone())
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])


def test_dk32_enters_the_function_only_when_a_gradient_is_asked_for(monkeypatch):
    """With is_cuda taken out of the question (a tensor subclass that claims the GPU): a frozen input through frozen weights takes the
    composition, the same call with a gradient asked for reaches the function, and with the switch off it does not."""
    from snuffy_amd import ssl_pretrain as S

    class OnGpu(torch.Tensor):
        is_cuda = True

        @classmethod
        def __torch_function__(cls, func, types, args=(), kwargs=None):
            return super().__torch_function__(func, types, args, kwargs or {})

    torch.manual_seed(1)
    attn = _Attn(64, 2)
    for p in attn.parameters():
        p.requires_grad = False
    entered = []
    monkeypatch.setattr(S, "FUSED_ATTENTION_DK32", True)
    monkeypatch.setattr(S.ViTAttentionFn, "apply", lambda qkv, b, t, h, scale: (entered.append((b, t, h)), qkv[:, :qkv.shape[1] // 3])[1])
    x = torch.randn(2, 37, 64).as_subclass(OnGpu)
    S._attention(attn, x)
    assert not entered
    S._attention(attn, x.clone().requires_grad_(True))
    assert entered == [(2, 37, 2)]
    monkeypatch.setattr(S, "FUSED_ATTENTION_DK32", False)
    S._attention(attn, x.clone().requires_grad_(True))
    assert entered == [(2, 37, 2)]


def test_dk32_kernels_keep_everything_in_registers():
    import scan_spills
    objdir = os.path.join(scan_spills.ROOT, "snuffy_amd", "build")
    if not os.path.isdir(objdir) or not any(f.endswith(".o") for f in os.listdir(objdir)):
        pytest.skip("no build objects here (the library was built elsewhere)")
    try:
        ks = scan_spills.kernels(objdir)
    except RuntimeError as exc:
        pytest.skip(str(exc))
    names = scan_spills.demangle([k[1] for k in ks])
    seen = {"vit_attn32_fwd_kernel<": 0, "vit_attn32_bwd_kernel<": 0, "vit_attn32_bwd_t1_kernel<": 0}
    bad = []
    for (obj, _, scratch, spilled, _vg), name in zip(ks, names):
        for key in seen:
            if key in name:
                seen[key] += 1
                if scratch or spilled:
                    bad.append((obj, name[:120], scratch, spilled))
    n = 2 * len(NKB_BUILT)
    assert seen == {"vit_attn32_fwd_kernel<": n, "vit_attn32_bwd_kernel<": n, "vit_attn32_bwd_t1_kernel<": 2}, seen
    assert not bad, bad
