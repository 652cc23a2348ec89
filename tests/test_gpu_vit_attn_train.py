"""Differentiable MFMA self-attention of adapter pre-training (csrc/vit.hip forward with lse, csrc/vit_attn_bwd.hip backward,
ssl_pretrain.ViTAttentionFn) on the GPU: the `short` row of tests/vit_attn_forms.py (dk = 64, T <= 256).  Both arithmetics against
float64 autograd, edges, refusals, saved state, and the block / DINO / MAE steps with the kernels engaged.  The shared bodies, the gates
and the figures behind them are in the table module; the forward's `torch.equal` with ops.vit_attention and the F11 DINO step are this
form's own."""
import numpy as np
import pytest
import torch

from tests import vit_attn_forms as V
from tests.helpers import DEV, _ops

pytestmark = pytest.mark.gpu
ROW = V.SHORT


@pytest.mark.parametrize("b,t,h", ROW.shapes + ROW.fwd_only)
@pytest.mark.parametrize("form", V.ARITHMETICS)
def test_forward_with_lse(form, b, t, h):
    qkv, _, _, lse_ref, _ = V.case(ROW, form, b, t, h)
    qd = qkv.to(DEV)
    out, lse = _ops().vit_attention_fwd_lse(qd, b, t, h, arithmetic=form)
    plain, _ = _ops().vit_attention(qd, b, t, h, arithmetic="x3" if form == "x3" else "exact")
    assert out.dtype == qkv.dtype and lse.dtype == torch.float32 and tuple(lse.shape) == (b, h, t)
    assert torch.equal(out, plain)                          # the same program: one more store, no other bit moves
    e = float((lse.cpu().double() - lse_ref).abs().max())
    print("MEASURED vit attention lse", form, (b, t, h), "abs err %.3e  (|lse| max %.2f)" % (e, float(lse_ref.abs().max())))
    assert e < ROW.lse_gate[form]


@pytest.mark.parametrize("b,t,h", ROW.shapes)
@pytest.mark.parametrize("form", V.ARITHMETICS)
def test_backward_against_float64(form, b, t, h):
    V.check_backward_against_float64(ROW, form, b, t, h)


@pytest.mark.parametrize("b,t,h", ROW.shapes)
@pytest.mark.parametrize("form", V.ARITHMETICS)
def test_backward_is_deterministic_and_writes_everything(form, b, t, h):
    V.check_backward_is_deterministic_and_writes_everything(ROW, form, b, t, h)


@pytest.mark.parametrize("form", V.ARITHMETICS)
def test_backward_stays_inside_its_buffers(form):
    V.check_kernels_stay_inside_their_buffers(ROW, form, *ROW.carve[0])


@pytest.mark.parametrize("form", V.ARITHMETICS)
def test_backward_refuses_what_it_does_not_serve(form):
    V.check_refuses_what_it_does_not_serve(ROW, form)


# ---- autograd layer ----------------------------------------------------------------------------------------------------------------------
def test_saved_state_is_qkv_and_one_float_per_row(monkeypatch):
    V.check_saved_state_is_qkv_and_one_float_per_row(monkeypatch, ROW)


def test_block_with_the_kernels_matches_the_composition(monkeypatch):
    V.check_block_with_the_kernels_matches_the_composition(monkeypatch, ROW, *ROW.blocks[0])


def test_dino_fixture_step_on_the_kernels(monkeypatch):
    """The DINO step of tests/test_gpu_vit.test_adapter_pretraining_steps_on_the_device with the switch forced on, against fixture F11
    and with that test's own tolerances."""
    from tests import test_ssl_pretrain as T
    S = V._ssl()
    monkeypatch.setattr(S, "FUSED_ATTENTION", True)
    fwd, bwd = V.count(monkeypatch, "vit_attention_fwd_lse"), V.count(monkeypatch, "vit_attention_bwd")
    z = T._npz("f11_dino_pretrain.npz")
    student, teacher = T._student(), T._student()
    student.load_state_dict(T._sd(z)), teacher.load_state_dict(T._sd(z))
    student, teacher = student.to(DEV).train(), teacher.to(DEV).train()
    for p in teacher.parameters():
        p.requires_grad = False
    S.freeze_for_adapter_tuning(student)
    crops = [torch.from_numpy(z[f"step_crop{i}"]).to(DEV) for i in range(4)]
    lm = S.DINOLoss(48, 4, 0.04, 0.07, 3, 10).to(DEV)
    with torch.no_grad():
        t_out = teacher(crops[:2])
    assert not fwd                                          # no gradient asked for: the composition
    loss = lm(student(crops), t_out, 1)
    loss.backward()
    # block 0 sees frozen tokens through frozen weights (nothing upstream needs a gradient); every later block engages, once per resolution
    resolutions = len({c.shape[-1] for c in crops})
    depth = len(student.backbone.blocks)
    assert resolutions == 2 and len(fwd) == len(bwd) == (depth - 1) * resolutions, (fwd, bwd)
    assert abs(float(loss.detach()) - float(z["step_loss"])) < 1e-4
    S.clip_gradients(student, 0.3)
    seen = 0
    for n, p in student.named_parameters():
        if p.grad is not None and "adaptmlp" in n:
            ref = z["grad." + n]
            assert np.allclose(p.grad.cpu().numpy(), ref, rtol=2e-3, atol=1e-3 * np.abs(ref).max() + 1e-7), n
            seen += 1
    assert seen >= 4


def test_mae_step_on_the_kernels(monkeypatch):
    V.check_mae_step_on_the_kernels(monkeypatch, ROW)


def test_autocast_runs_the_bf16_kernels(monkeypatch):
    V.check_autocast_runs_the_bf16_kernels(monkeypatch, ROW)
