"""Host side of the differentiable ViT self-attention (no GPU), over the table of tests/vit_attn_forms.py: the form table of ops.py
against the shape predicates and the header, the routing of ssl_pretrain._attention away from and into ViTAttentionFn, the float64
yardstick of the GPU suite at the long form's shapes, and the registers of the built kernels."""
import os
import re

import pytest
import torch

from tests import vit_attn_forms as V
from tests.vit_attn_forms import DK32, LONG, ROWS, SHORT


def test_predicates_and_the_lookup_are_the_form_table():
    """short: dk = 64 and one LDS image of keys; long: dk = 64 above it, up to 4096; dk32: dk = 32 and T <= 256.  No shape has two
    forms, and the lookup names the form whose predicate holds."""
    from snuffy_amd import ops
    assert (ops.VIT_BWD_MAX_T, ops.VIT_BWD_LONG_MAX_T, ops.VIT_DK32_MAX_T) == (256, 4096, 256)
    for dk in (16, 32, 64, 128):
        for t in range(0, 4200):
            short, long_, dk32 = (ops.vit_attention_bwd_supported(t, dk), ops.vit_attention_bwd_long_supported(t, dk),
                                  ops.vit_attention_dk32_supported(t, dk))
            assert short is (dk == 64 and 1 <= t <= 256), (t, dk)
            assert long_ is (dk == 64 and 256 < t <= 4096), (t, dk)
            assert dk32 is (dk == 32 and 1 <= t <= 256), (t, dk)
            form = ops.vit_attention_train_form(t, dk)
            assert (form and form.name) == ("short" if short else "long" if long_ else "dk32" if dk32 else None), (t, dk)
    for row, form in zip(ROWS, ops.VIT_TRAIN_FORMS):        # the tests' records name what the product's do
        assert (row.name, row.dk, row.fwd, row.bwd, row.c_fwd, row.c_bwd) == (form.name, form.dk, form.fwd, form.bwd, form.c_fwd, form.c_bwd)
        assert row.switch == V._ssl().FORM_SWITCH[form.name]


def test_bounds_are_the_headers():
    """The four SNF_VIT_*_MAX_T of include/snuffy_hip.h against the table of ops.py and the public constants."""
    from snuffy_amd import ops
    text = open(os.path.join(V.ROOT, "include", "snuffy_hip.h")).read()
    defines = {k: int(v) for k, v in re.findall(r"^#define (SNF_VIT_\w*MAX_T) (\d+)\s*$", text, re.M)}
    short, long_, dk32 = ops.VIT_TRAIN_FORMS
    assert defines == {"SNF_VIT_MFMA_MAX_T": ops.VIT_MFMA_MAX_T, "SNF_VIT_BWD_MAX_T": ops.VIT_BWD_MAX_T,
                       "SNF_VIT_BWD_LONG_MAX_T": ops.VIT_BWD_LONG_MAX_T, "SNF_VIT_DK32_MAX_T": ops.VIT_DK32_MAX_T}
    assert (short.t_max, long_.t_max, dk32.t_max) == (defines["SNF_VIT_BWD_MAX_T"], defines["SNF_VIT_BWD_LONG_MAX_T"], defines["SNF_VIT_DK32_MAX_T"])
    assert (short.t_min, long_.t_min, dk32.t_min) == (1, defines["SNF_VIT_BWD_MAX_T"] + 1, 1)
    assert defines["SNF_VIT_MFMA_MAX_T"] == max(f.t_max for f in ops.VIT_TRAIN_FORMS if f.fwd == "vit_attention_fwd_lse")


def _never(*args, **kw):
    raise AssertionError("ViTAttentionFn was entered")


@pytest.mark.parametrize("row", V.by_row(ROWS))
def test_cpu_tensors_take_the_composition_bit_for_bit(monkeypatch, row):
    S = V._ssl()
    torch.manual_seed(0)
    attn = V.Attn(row.host.x[2], row.host.h)
    x = torch.randn(*row.host.x, requires_grad=True)
    monkeypatch.setattr(S.ViTAttentionFn, "apply", _never)
    for name in row.host.hold:
        monkeypatch.setattr(S, name, True)
    res = {}
    for flag in (True, False):
        monkeypatch.setattr(S, row.switch, flag)
        x.grad = None
        y = S._attention(attn, x)
        y.square().sum().backward()
        res[flag] = (y.detach().clone(), x.grad.clone())
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])


@pytest.mark.parametrize("row", V.by_row([SHORT, DK32]))
def test_no_gradient_asked_for_means_no_autograd_function(monkeypatch, row):
    """The condition is on qkv.requires_grad: with is_cuda taken out of the question (a tensor subclass that claims the GPU), a frozen
    input through frozen weights still takes the composition, and the same call with a gradient asked for reaches the function -- and
    (dk32) with the switch off it does not."""
    S = V._ssl()
    torch.manual_seed(1)
    b, t, d = row.host.x
    attn = V.Attn(d, row.host.h)
    for p in attn.parameters():
        p.requires_grad = False
    entered = []
    monkeypatch.setattr(S, row.switch, True)
    monkeypatch.setattr(S.ViTAttentionFn, "apply", lambda qkv, b, t, h, scale: (entered.append((b, t, h)), qkv[:, :qkv.shape[1] // 3])[1])
    x = torch.randn(b, t, d).as_subclass(V.OnGpu)
    S._attention(attn, x)
    assert not entered
    S._attention(attn, x.clone().requires_grad_(True))
    assert entered == [(b, t, row.host.h)]
    if row in (DK32,):
        monkeypatch.setattr(S, row.switch, False)
        S._attention(attn, x.clone().requires_grad_(True))
        assert entered == [(b, t, row.host.h)]


def test_a_gradient_on_the_gpu_reaches_the_function_only_with_the_switch(monkeypatch):
    """With is_cuda taken out of the question (a tensor subclass that claims the GPU): T = 300 enters ViTAttentionFn with the long switch
    on whatever the short switch says, and takes the composition with it off."""
    S = V._ssl()
    torch.manual_seed(1)
    b, t, d = LONG.host.x
    attn = V.Attn(d, LONG.host.h)
    entered = []
    monkeypatch.setattr(S.ViTAttentionFn, "apply", lambda qkv, b, t, h, scale: (entered.append((b, t, h)), qkv[:, :qkv.shape[1] // 3])[1])
    x = torch.randn(b, t, d).as_subclass(V.OnGpu).requires_grad_(True)
    for short, long_, expect in ((True, False, []), (False, False, []), (False, True, [(1, 300, 2)]), (True, True, [(1, 300, 2)])):
        monkeypatch.setattr(S, "FUSED_ATTENTION", short)
        monkeypatch.setattr(S, "FUSED_ATTENTION_LONG", long_)
        del entered[:]
        S._attention(attn, x)
        assert entered == expect, (short, long_)


def test_float64_yardstick_is_sane_at_the_gpu_suites_shapes():
    """Every table entry of the long form: finite operands and float64 gradients, no zero-norm third."""
    for form in V.ARITHMETICS:
        for b, t, h in LONG.shapes:
            qkv, dout, _, lse, dref = V.case(LONG, form, b, t, h)
            assert qkv.shape == (b * t, 3 * h * 64) and dout.shape == (b * t, h * 64) and lse.shape == (b, h, t)
            assert bool(torch.isfinite(lse).all()) and dref.dtype == torch.float64
            for name, third in V.thirds(dref):
                assert bool(torch.isfinite(third).all()) and float(third.norm()) > 0, (form, b, t, h, name)


@pytest.mark.parametrize("row", V.by_row(ROWS))
def test_kernels_keep_everything_in_registers(row):
    seen, bad = V.scan_registers(row)
    assert seen == row.kernels, seen
    assert not bad, bad
