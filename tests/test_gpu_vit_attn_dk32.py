"""Differentiable MFMA self-attention at head width 32 (csrc/vit_attn_dk32.hip: forward with lse and backward, T <= 256; the MAE
decoder of adapter pre-training through ssl_pretrain.ViTAttentionFn) on the GPU: the `dk32` row of tests/vit_attn_forms.py.  Both
arithmetics against float64 autograd of the composition computed on the CPU, edges, refusals, saved state, and a MAE step whose decoder
runs these kernels.  The shared bodies, the gates and the figures behind them are in the table module; the forward against float64 with
its `out` gate is this form's own."""
import pytest
import torch

from tests import vit_attn_forms as V
from tests.helpers import DEV, _ops, rel_err

pytestmark = pytest.mark.gpu
ROW = V.DK32


@pytest.mark.parametrize("b,t,h", ROW.shapes)
@pytest.mark.parametrize("form", V.ARITHMETICS)
def test_forward_against_float64(form, b, t, h):
    qkv, _, out_ref, lse_ref, _ = V.case(ROW, form, b, t, h)
    qd = qkv.to(DEV)
    out, lse = _ops().vit_attention_dk32_fwd_lse(qd, b, t, h, arithmetic=form)
    assert out.dtype == qkv.dtype and tuple(out.shape) == (b * t, h * ROW.dk)
    assert lse.dtype == torch.float32 and tuple(lse.shape) == (b, h, t)
    comp = V.composition(qd, b, t, h)[0]                    # the same dtype on the device: not a yardstick, printed for scale
    e_out, e_comp = rel_err(out.cpu(), out_ref), rel_err(comp.cpu(), out_ref)
    e_lse = float((lse.cpu().double() - lse_ref).abs().max())
    print("MEASURED vit attention dk32 fwd", form, (b, t, h), "out kernel %.3e  torch composition %.3e  lse abs err %.3e  (|lse| max %.2f)"
          % (e_out, e_comp, e_lse, float(lse_ref.abs().max())))
    assert e_lse < ROW.lse_gate[form]
    assert e_out < ROW.out_gate[form]


@pytest.mark.parametrize("b,t,h", ROW.shapes)
@pytest.mark.parametrize("form", V.ARITHMETICS)
def test_backward_against_float64(form, b, t, h):
    V.check_backward_against_float64(ROW, form, b, t, h)


@pytest.mark.parametrize("b,t,h", ROW.shapes)
@pytest.mark.parametrize("form", V.ARITHMETICS)
def test_backward_is_deterministic_and_writes_everything(form, b, t, h):
    V.check_backward_is_deterministic_and_writes_everything(ROW, form, b, t, h)


@pytest.mark.parametrize("form", V.ARITHMETICS)
def test_both_kernels_stay_inside_their_buffers(form):
    V.check_kernels_stay_inside_their_buffers(ROW, form, *ROW.carve[0])


@pytest.mark.parametrize("form", V.ARITHMETICS)
def test_refuses_what_it_does_not_serve(form):
    V.check_refuses_what_it_does_not_serve(ROW, form)


# ---- autograd layer ----------------------------------------------------------------------------------------------------------------------
def test_mae_step_runs_its_decoder_on_the_dk32_kernels(monkeypatch):
    V.check_mae_step_on_the_kernels(monkeypatch, ROW)


def test_saved_state_is_qkv_and_one_float_per_row(monkeypatch):
    V.check_saved_state_is_qkv_and_one_float_per_row(monkeypatch, ROW)


def test_autocast_runs_the_bf16_kernels(monkeypatch):
    V.check_autocast_runs_the_bf16_kernels(monkeypatch, ROW)
