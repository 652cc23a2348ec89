"""Backward of the MFMA ViT self-attention above 256 tokens (csrc/vit_attn_bwd_long.hip: a dQ launch over key chunks and a dK / dV launch
over query chunks, ops.vit_attention_bwd_long, ssl_pretrain.FUSED_ATTENTION_LONG) on the GPU: the `long` row of tests/vit_attn_forms.py.
Both arithmetics against float64 autograd at the shapes where the chunk walk can go wrong, determinism, buffer edges, refusals, and the
autograd layer with the switch on and off.  The shared bodies, the gates and the figures behind them are in the table module; the
independence of images and heads is this form's own."""
import pytest
import torch

from tests import vit_attn_forms as V
from tests.helpers import DEV, _ops

pytestmark = pytest.mark.gpu
ROW = V.LONG


@pytest.mark.parametrize("b,t,h", ROW.shapes)
@pytest.mark.parametrize("form", V.ARITHMETICS)
def test_backward_against_float64(form, b, t, h):
    V.check_backward_against_float64(ROW, form, b, t, h)


@pytest.mark.parametrize("b,t,h", ROW.shapes)
@pytest.mark.parametrize("form", V.ARITHMETICS)
def test_backward_is_deterministic_and_writes_everything(form, b, t, h):
    V.check_backward_is_deterministic_and_writes_everything(ROW, form, b, t, h)


@pytest.mark.parametrize("b,t,h", ROW.carve)
@pytest.mark.parametrize("form", V.ARITHMETICS)
def test_backward_stays_inside_its_buffers_and_padding_never_leaks(form, b, t, h):
    V.check_kernels_stay_inside_their_buffers(ROW, form, b, t, h)


@pytest.mark.parametrize("form", V.ARITHMETICS)
def test_images_and_heads_are_independent(form):
    b, t, h = 2, 785, 2
    qkv, dout, _, _, _ = V.case(ROW, form, b, t, h)
    qd, dd = qkv.to(DEV), dout.to(DEV)
    lse = _ops().vit_attention_fwd_lse(qd, b, t, h)[1]
    full = _ops().vit_attention_bwd_long(qd, dd, lse, b, t, h)
    # image 1, head 1 as a (1, 785, 1) problem on that slice's operands
    q1 = qd.view(b, t, 3, h, 64)[1, :, :, 1].reshape(t, 192).contiguous()
    d1 = dd.view(b, t, h, 64)[1, :, 1].contiguous()
    l1 = lse[1:2, 1:2].contiguous()
    alone = _ops().vit_attention_bwd_long(q1, d1, l1, 1, t, 1)
    assert torch.equal(full.view(b, t, 3, h, 64)[1, :, :, 1].reshape(t, 192), alone)


@pytest.mark.parametrize("form", V.ARITHMETICS)
def test_backward_refuses_what_it_does_not_serve(form):
    V.check_refuses_what_it_does_not_serve(ROW, form)


# ---- autograd layer ----------------------------------------------------------------------------------------------------------------------
def test_saved_state_is_qkv_and_one_float_per_row(monkeypatch):
    V.check_saved_state_is_qkv_and_one_float_per_row(monkeypatch, ROW)


@pytest.mark.parametrize("b,t,d,h,bott", ROW.blocks, ids=[str(dims[1]) for dims in ROW.blocks])
def test_block_with_the_kernels_matches_the_composition(monkeypatch, b, t, d, h, bott):
    V.check_block_with_the_kernels_matches_the_composition(monkeypatch, ROW, b, t, d, h, bott)


def test_autocast_runs_the_bf16_kernels(monkeypatch):
    V.check_autocast_runs_the_bf16_kernels(monkeypatch, ROW)
