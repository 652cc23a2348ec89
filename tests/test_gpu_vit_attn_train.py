"""Differentiable MFMA self-attention of adapter pre-training (csrc/vit.hip forward with lse, csrc/vit_attn_bwd.hip backward,
ssl_pretrain.ViTAttentionFn) on the GPU: both arithmetics against float64 autograd, edges, refusals, saved state, and the block /
DINO / MAE steps with the kernels engaged.

Measured on an MI355X (profiles/vit_attn_train.txt has every figure), largest over the table, and the gates chosen from it:
  lse |err| vs float64      fp32 class 5.2e-5 (the x3 scores' own error at |scale s| ~ 11) -> 4 x is above the cap: gate 1e-4;
                            bf16 1.3e-6 -> 4 x, one digit: 6e-6 (cap 5e-2)
  dQ / dK / dV rel_err      fp32 class 2.1e-5 -> 4 x, one digit: 9e-5 (cap 2e-4);  bf16 6.6e-3 -> 2 x, one digit: 2e-2 (cap 3e-2)
  the torch composition of the same dtype on the same inputs: fp32 2.2e-7 ... 1.4e-6, bf16 4.0e-3 ... 1.1e-2
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import rel_err, vit_block_state

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16

FORMS = ("x3", "bf16")
SHAPES = [(1, 1, 1), (2, 17, 1), (2, 32, 2), (2, 33, 1), (2, 37, 2), (3, 50, 3), (2, 197, 6), (2, 224, 2), (2, 225, 2), (2, 256, 2)]
FWD_ONLY = [(2, 785, 2), (1, 257, 2)]           # the chunked forms emit lse too
LSE_GATE = {"x3": 1e-4, "bf16": 6e-6}           # absolute; caps of the issue: 1e-4 / 5e-2
BWD_GATE = {"x3": 9e-5, "bf16": 2e-2}         # tests.helpers.rel_err; caps of the issue: 2e-4 / 3e-2


def _ops():
    from snuffy_amd import ops
    return ops


def _ssl():
    from snuffy_amd import ssl_pretrain
    return ssl_pretrain


def _composition(qkv, b, t, h):
    """The composition of tests/test_gpu_vit.ref_attention, in the dtype of qkv -> (out [b*t, d], scores * scale)."""
    d = qkv.shape[1] // 3
    dk = d // h
    q, k, v = qkv.view(b, t, 3, h, dk).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-2, -1)) * dk ** -0.5
    return (s.softmax(-1) @ v).transpose(1, 2).reshape(b * t, d), s


@functools.lru_cache(maxsize=None)
def _case(form, b, t, h):
    """Operands of one table row (host tensors in the form's dtype) and the float64 yardstick computed from those operands: out, lse,
    dQ | dK | dV.  Computed once per row and shared; nothing writes to it."""
    g = torch.Generator().manual_seed(1000 * t + 10 * h + b)
    qkv = torch.randn(b * t, 3 * h * 64, generator=g) * 1.5
    dout = torch.randn(b * t, h * 64, generator=g)
    if form == "bf16":
        qkv, dout = qkv.to(BF), dout.to(BF)
    q64 = qkv.double().requires_grad_(True)
    out, s = _composition(q64, b, t, h)
    out.backward(dout.double())
    return qkv, dout, out.detach(), torch.logsumexp(s.detach(), -1), q64.grad


def _thirds(dqkv):
    d = dqkv.shape[1] // 3
    return (("dQ", dqkv[:, :d]), ("dK", dqkv[:, d:2 * d]), ("dV", dqkv[:, 2 * d:]))


@pytest.mark.parametrize("b,t,h", SHAPES + FWD_ONLY)
@pytest.mark.parametrize("form", FORMS)
def test_forward_with_lse(form, b, t, h):
    qkv, _, _, lse_ref, _ = _case(form, b, t, h)
    qd = qkv.to(DEV)
    out, lse = _ops().vit_attention_fwd_lse(qd, b, t, h, arithmetic=form)
    plain, _ = _ops().vit_attention(qd, b, t, h, arithmetic="x3" if form == "x3" else "exact")
    assert out.dtype == qkv.dtype and lse.dtype == torch.float32 and tuple(lse.shape) == (b, h, t)
    assert torch.equal(out, plain)                          # the same program: one more store, no other bit moves
    e = float((lse.cpu().double() - lse_ref).abs().max())
    print("MEASURED vit attention lse", form, (b, t, h), "abs err %.3e  (|lse| max %.2f)" % (e, float(lse_ref.abs().max())))
    assert e < LSE_GATE[form]


@pytest.mark.parametrize("b,t,h", SHAPES)
@pytest.mark.parametrize("form", FORMS)
def test_backward_against_float64(form, b, t, h):
    qkv, dout, _, _, dref = _case(form, b, t, h)
    qd, dd = qkv.to(DEV), dout.to(DEV)
    _, lse = _ops().vit_attention_fwd_lse(qd, b, t, h)
    dqkv = _ops().vit_attention_bwd(qd, dd, lse, b, t, h)
    assert dqkv.dtype == qkv.dtype and dqkv.shape == qkv.shape
    # the torch composition in the same dtype on the same device: not a yardstick, printed for scale
    qc = qd.clone().requires_grad_(True)
    _composition(qc, b, t, h)[0].backward(dd)
    errs = []
    for (name, got), (_, comp), (_, want) in zip(_thirds(dqkv.cpu()), _thirds(qc.grad.cpu()), _thirds(dref)):
        if t == 1 and name != "dV":
            assert not bool(got.any()) and not bool(want.any())
            continue
        e = rel_err(got, want)
        errs.append(e)
        print("MEASURED vit attention bwd", form, (b, t, h), name, "kernel %.3e  torch composition %.3e" % (e, rel_err(comp, want)))
    assert max(errs) < BWD_GATE[form], errs


@pytest.mark.parametrize("b,t,h", SHAPES)
@pytest.mark.parametrize("form", FORMS)
def test_backward_is_deterministic_and_writes_everything(form, b, t, h):
    qkv, dout, _, _, _ = _case(form, b, t, h)
    qd, dd = qkv.to(DEV), dout.to(DEV)
    _, lse = _ops().vit_attention_fwd_lse(qd, b, t, h)
    first = torch.full_like(qd, float("nan"))
    second = torch.full_like(qd, float("nan"))
    assert _ops().vit_attention_bwd(qd, dd, lse, b, t, h, out=first) is first
    _ops().vit_attention_bwd(qd, dd, lse, b, t, h, out=second)
    assert not bool(torch.isnan(first).any())
    assert torch.equal(first, second)
    if t == 1:      # softmax over one key is the constant 1: nothing flows to q and k, dout passes to v unchanged
        d = h * 64
        assert not bool(first[:, :2 * d].any()) and torch.equal(first[:, 2 * d:], dd)


@pytest.mark.parametrize("form", FORMS)
def test_backward_stays_inside_its_buffers(form):
    b, t, h = 2, 37, 2
    qkv, dout, _, _, _ = _case(form, b, t, h)
    pad = 256                                               # elements: keeps the carved tensors 16-byte aligned

    def carve(src):
        buf = torch.full((src.numel() + 2 * pad,), float("nan"), dtype=src.dtype, device=DEV)
        view = buf[pad:pad + src.numel()].view(src.shape)
        view.copy_(src)
        return buf, view

    qbuf, qd = carve(qkv)
    dbuf, dd = carve(dout)
    _, lse = _ops().vit_attention_fwd_lse(qkv.to(DEV), b, t, h)
    lbuf, ld = carve(lse)
    obuf, od = carve(torch.zeros_like(qkv))
    od.fill_(float("nan"))
    _ops().vit_attention_bwd(qd, dd, ld, b, t, h, out=od)
    want = _ops().vit_attention_bwd(qkv.to(DEV), dout.to(DEV), lse, b, t, h)
    assert torch.equal(od, want)
    for buf in (qbuf, dbuf, lbuf, obuf):
        assert bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[-pad:]).all())
    assert torch.equal(qd, qkv.to(DEV)) and torch.equal(dd, dout.to(DEV))       # inputs untouched


@pytest.mark.parametrize("form", FORMS)
def test_backward_refuses_what_it_does_not_serve(form):
    ops = _ops()
    dt = torch.float32 if form == "x3" else BF

    def call(b, t, h, dk, shift=0):
        n = b * t * 3 * h * dk
        qkv = torch.zeros(n + 8, dtype=dt, device=DEV)[shift:shift + n].view(b * t, 3 * h * dk)
        dout = torch.zeros(b * t, h * dk, dtype=dt, device=DEV)
        lse = torch.zeros(b, h, t, dtype=torch.float32, device=DEV)
        return ops.vit_attention_bwd(qkv, dout, lse, b, t, h)

    assert call(1, 256, 1, 64).shape == (256, 192)          # the edge of the domain is served
    assert ops.vit_attention_bwd_supported(256, 64)
    for kw, supported in ((dict(t=257, dk=64), False), (dict(t=8, dk=32), False), (dict(t=8, dk=64, shift=1), True)):
        assert ops.vit_attention_bwd_supported(kw["t"], kw["dk"]) is supported
        with pytest.raises(ops._ffi.SnuffyHipError, match=r"code -3\): snf_vit_attention_bwd: unsupported"):
            call(1, kw["t"], 2, kw["dk"], kw.get("shift", 0))
    with pytest.raises(ops._ffi.SnuffyHipError, match="GPU tensor"):
        ops.vit_attention_bwd(torch.zeros(8, 192), torch.zeros(8, 64), torch.zeros(1, 1, 8), 1, 8, 1)
    with pytest.raises(ops._ffi.SnuffyHipError, match="GPU tensor"):
        ops.vit_attention_fwd_lse(torch.zeros(8, 192), 1, 8, 1)


# ---- autograd layer ----------------------------------------------------------------------------------------------------------------------
def _count(monkeypatch, name):
    """Wrap ops.<name> in a recorder of its (qkv shape, heads) -> the list."""
    ops = _ops()
    calls, real = [], getattr(ops, name)

    def wrapped(qkv, *args, **kw):
        calls.append((tuple(qkv.shape), args[4] if name == "vit_attention_bwd" else args[2]))
        return real(qkv, *args, **kw)

    monkeypatch.setattr(ops, name, wrapped)
    return calls


def _vit(embed, heads, depth, bott=64, seed=0):
    from snuffy_amd import vit
    model = vit.VisionTransformer(img_size=[224], patch_size=16, embed_dim=embed, depth=depth, num_heads=heads, mlp_ratio=4, qkv_bias=True,
                                  norm_layer=functools.partial(torch.nn.LayerNorm, eps=1e-6), adapter_ffn_layernorm_option="none",
                                  adapter_ffn_init_option="lora", adapter_ffn_scalar="0.1", adapter_ffn_num=bott, adapter_d_model=embed)
    missing = model.load_state_dict(vit_block_state(embed, depth, bott, seed=seed), strict=False)
    assert not [k for k in missing.missing_keys if k.startswith("blocks.")] and not missing.unexpected_keys
    for m in model.modules():
        if isinstance(getattr(m, "dropout", None), float):
            m.dropout = 0.0
    return model.to(DEV).train()


def test_saved_state_is_qkv_and_one_float_per_row(monkeypatch):
    S = _ssl()
    b, t, h = 2, 197, 6
    attn = _vit(384, h, 1).blocks[0].attn
    x = torch.randn(b, t, 384, device=DEV, generator=torch.Generator(DEV).manual_seed(3), requires_grad=True)
    saved = []

    def run(fn):
        del saved[:]
        with torch.autograd.graph.saved_tensors_hooks(lambda ten: (saved.append(ten), ten)[1], lambda ten: ten):
            return fn()

    qkv = F.linear(x, attn.qkv.weight, attn.qkv.bias).view(b * t, 3 * 384)
    out = run(lambda: S.ViTAttentionFn.apply(qkv, b, t, h, attn.scale))
    assert len(saved) == 2
    assert saved[0].data_ptr() == qkv.data_ptr() and saved[0].shape == qkv.shape
    assert saved[1].dtype == torch.float32 and saved[1].numel() == b * h * t
    out.sum().backward()
    assert x.grad is not None and bool(torch.isfinite(x.grad).all())
    for flag, expect in ((True, False), (False, True)):
        monkeypatch.setattr(S, "FUSED_ATTENTION", flag)
        run(lambda: S._attention(attn, x))
        assert any(ten.numel() == b * h * t * t for ten in saved) is expect, (flag, [tuple(ten.shape) for ten in saved])


def test_block_with_the_kernels_matches_the_composition(monkeypatch):
    S = _ssl()
    b, t, d, h = 2, 197, 384, 6
    blk = _vit(d, h, 1).blocks[0]
    g = torch.Generator().manual_seed(5)
    x0, dy = torch.randn(b, t, d, generator=g).to(DEV), torch.randn(b, t, d, generator=g).to(DEV)
    calls = _count(monkeypatch, "vit_attention_bwd")
    res = {}
    for flag in (True, False):
        monkeypatch.setattr(S, "FUSED_ATTENTION", flag)
        blk.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        y = S.block_autograd(blk, x, True)
        y.backward(dy)
        res[flag] = [("y", y.detach()), ("dx", x.grad)] + [(n, p.grad.clone()) for n, p in blk.adaptmlp.named_parameters() if p.grad is not None and p.numel() > 1]
        assert len(calls) == 1, (flag, calls)               # once with the switch on, not at all with it off
    assert len(res[True]) == 6                              # output, d/dx, the adapter's two weights and two biases
    for (name, on), (_, off) in zip(res[True], res[False]):
        e = rel_err(on, off)
        print("MEASURED vit attention block on vs off", name, "%.3e" % e)
        assert e < 2e-4, name


def test_dino_fixture_step_on_the_kernels(monkeypatch):
    """The DINO step of tests/test_gpu_vit.test_adapter_pretraining_steps_on_the_device with the switch forced on, against fixture F11
    and with that test's own tolerances."""
    from tests import test_ssl_pretrain as T
    S = _ssl()
    monkeypatch.setattr(S, "FUSED_ATTENTION", True)
    fwd, bwd = _count(monkeypatch, "vit_attention_fwd_lse"), _count(monkeypatch, "vit_attention_bwd")
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
    S = _ssl()
    torch.manual_seed(12)
    model = S.MAEPretrainModel(img_size=64, patch_size=16, embed_dim=128, depth=2, num_heads=2, decoder_embed_dim=32, decoder_depth=1,
                               decoder_num_heads=2, mlp_ratio=4, norm_layer=functools.partial(torch.nn.LayerNorm, eps=1e-6),
                               norm_pix_loss=True, adapter_ffn_scalar="1.0", adapter_ffn_num=8, adapter_d_model=128)
    g = torch.Generator().manual_seed(13)
    with torch.no_grad():
        for n, p in model.named_parameters():               # nothing at its init value (the LoRA zero init would hide the adapters)
            if p.requires_grad and "adaptmlp" in n:
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    for m in model.modules():
        if isinstance(getattr(m, "dropout", None), float):
            m.dropout = 0.0
    model = model.to(DEV).train()
    imgs = torch.rand(4, 3, 64, 64, generator=g).to(DEV)
    noise = torch.rand(4, 16, generator=g).to(DEV)
    bwd = _count(monkeypatch, "vit_attention_bwd")
    res = {}
    for flag in (True, False):
        monkeypatch.setattr(S, "FUSED_ATTENTION", flag)
        model.zero_grad(set_to_none=True)
        loss, _, _ = model(imgs, 0.75, noise)
        loss.backward()
        res[flag] = (float(loss), {n: p.grad.clone() for n, p in model.named_parameters() if "adaptmlp" in n and p.grad is not None})
        # the two encoder blocks (dk = 64, T = 1 + 4 kept patches) ran on the kernel, the decoder block (dk = 16) did not
        assert bwd == [((4 * 5, 3 * 128), 2)] * 2, (flag, bwd)
    assert abs(res[True][0] - res[False][0]) < 1e-5
    assert len(res[True][1]) >= 12
    for n, on in res[True][1].items():
        e = rel_err(on, res[False][1][n])
        print("MEASURED vit attention mae on vs off", n, "%.3e" % e)
        assert e < 2e-4, n


def test_autocast_runs_the_bf16_kernels(monkeypatch):
    """The form follows the dtype of the qkv Linear's output: under torch.autocast(bfloat16) both kernels get bf16 tensors."""
    S, ops = _ssl(), _ops()
    b, t, h = 2, 37, 2
    attn = _vit(128, h, 1, bott=8).blocks[0].attn
    seen = []
    real_f, real_b = ops.vit_attention_fwd_lse, ops.vit_attention_bwd
    monkeypatch.setattr(ops, "vit_attention_fwd_lse", lambda qkv, *a, **k: (seen.append(("fwd", qkv.dtype)), real_f(qkv, *a, **k))[1])
    monkeypatch.setattr(ops, "vit_attention_bwd", lambda qkv, dout, *a, **k: (seen.append(("bwd", qkv.dtype, dout.dtype)), real_b(qkv, dout, *a, **k))[1])
    monkeypatch.setattr(S, "FUSED_ATTENTION", True)
    x = torch.randn(b, t, 128, device=DEV, generator=torch.Generator(DEV).manual_seed(9), requires_grad=True)
    with torch.autocast("cuda", BF):
        y = S._attention(attn, x)
    y.float().sum().backward()
    assert seen == [("fwd", BF), ("bwd", BF, BF)]
    assert y.dtype == BF and x.grad.dtype == torch.float32 and bool(torch.isfinite(x.grad).all()) and bool(x.grad.any())
