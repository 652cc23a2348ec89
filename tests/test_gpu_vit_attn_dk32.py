"""Differentiable MFMA self-attention at head width 32 (csrc/vit_attn_dk32.hip: forward with lse and backward, T <= 256; the MAE
decoder of adapter pre-training through ssl_pretrain.ViTAttentionFn) on the GPU: both arithmetics against float64 autograd of the
composition computed on the CPU, edges, refusals, saved state, and a MAE step whose decoder runs the new kernels.

Measured on an MI355X (profiles/vit_attn_dk32_train.txt has every figure), largest over the table, and the gates chosen from it:
  lse |err| vs float64      fp32 class 5.1e-5 -> 4 x is above the cap, so the gate is the cap: 1e-4.  The figure is the x3 scores' own
                            error, not the kernel's: q and k are each hi + lo with lo rounded to bf16 and lo lo dropped (about 2^-17
                            relative per operand), and scale * sum |q_i k_i| is about 8 at these operands, so 6e-5 is what the
                            arithmetic allows; the 64-wide pair measures 5.2e-5 on the same distribution.
                            bf16 1.22e-6 -> 2 x = 2.4e-6, one digit up: 3e-6 (cap 5e-2)
  dQ / dK / dV rel_err      fp32 class 3.1e-5 -> 4 x = 1.24e-4, one digit up: 2e-4 (the cap);  bf16 5.6e-3 -> 2 x = 1.1e-2, one digit
                            up: 2e-2 (cap 3e-2)
  out rel_err               fp32 class 1.64e-5 (torch fp32 composition 9.8e-7) -> 4 x the larger = 6.6e-5, one digit up: 7e-5
                            bf16 3.5e-3 (torch bf16 composition 1.86e-2) -> 2 x the larger = 3.7e-2, one digit up: 4e-2
  the torch composition of the same dtype on the same inputs, backward: fp32 2.6e-7 ... 8.9e-7, bf16 5.0e-3 ... 2.0e-2
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
DK = 32

FORMS = ("x3", "bf16")
# (b, t, h): the copy kernel; under one tile; the tile edge and an odd head count; ragged tiles; NKB = 4 (100); the decoder's own T
# and h; the last key block whole, one past it, and the edge of the domain
SHAPES = [(1, 1, 1), (2, 17, 1), (2, 32, 2), (2, 33, 3), (2, 37, 2), (3, 50, 3), (1, 100, 2), (1, 197, 16), (2, 224, 2), (2, 225, 2),
          (2, 256, 2)]
LSE_GATE = {"x3": 1e-4, "bf16": 3e-6}           # absolute; caps of the 64-wide pair: 1e-4 / 5e-2
BWD_GATE = {"x3": 2e-4, "bf16": 2e-2}           # tests.helpers.rel_err; caps of the 64-wide pair: 2e-4 / 3e-2
OUT_GATE = {"x3": 7e-5, "bf16": 4e-2}           # tests.helpers.rel_err; 4 x / 2 x the larger of kernel and torch composition


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
    """Operands of one table row (host tensors in the form's dtype) and the float64 yardstick computed from those operands on the CPU:
    out, lse, dQ | dK | dV.  Computed once per row and shared; nothing writes to it."""
    g = torch.Generator().manual_seed(1000 * t + 10 * h + b)
    qkv = torch.randn(b * t, 3 * h * DK, generator=g) * 1.5
    dout = torch.randn(b * t, h * DK, generator=g)
    if form == "bf16":
        qkv, dout = qkv.to(BF), dout.to(BF)
    q64 = qkv.double().requires_grad_(True)
    out, s = _composition(q64, b, t, h)
    out.backward(dout.double())
    return qkv, dout, out.detach(), torch.logsumexp(s.detach(), -1), q64.grad


def _thirds(dqkv):
    d = dqkv.shape[1] // 3
    return (("dQ", dqkv[:, :d]), ("dK", dqkv[:, d:2 * d]), ("dV", dqkv[:, 2 * d:]))


@pytest.mark.parametrize("b,t,h", SHAPES)
@pytest.mark.parametrize("form", FORMS)
def test_forward_against_float64(form, b, t, h):
    qkv, _, out_ref, lse_ref, _ = _case(form, b, t, h)
    qd = qkv.to(DEV)
    out, lse = _ops().vit_attention_dk32_fwd_lse(qd, b, t, h, arithmetic=form)
    assert out.dtype == qkv.dtype and tuple(out.shape) == (b * t, h * DK)
    assert lse.dtype == torch.float32 and tuple(lse.shape) == (b, h, t)
    comp = _composition(qd, b, t, h)[0]                     # the same dtype on the device: not a yardstick, printed for scale
    e_out, e_comp = rel_err(out.cpu(), out_ref), rel_err(comp.cpu(), out_ref)
    e_lse = float((lse.cpu().double() - lse_ref).abs().max())
    print("MEASURED vit attention dk32 fwd", form, (b, t, h), "out kernel %.3e  torch composition %.3e  lse abs err %.3e  (|lse| max %.2f)"
          % (e_out, e_comp, e_lse, float(lse_ref.abs().max())))
    assert e_lse < LSE_GATE[form]
    assert e_out < OUT_GATE[form]


@pytest.mark.parametrize("b,t,h", SHAPES)
@pytest.mark.parametrize("form", FORMS)
def test_backward_against_float64(form, b, t, h):
    qkv, dout, _, _, dref = _case(form, b, t, h)
    qd, dd = qkv.to(DEV), dout.to(DEV)
    _, lse = _ops().vit_attention_dk32_fwd_lse(qd, b, t, h)
    dqkv = _ops().vit_attention_dk32_bwd(qd, dd, lse, b, t, h)
    assert dqkv.dtype == qkv.dtype and dqkv.shape == qkv.shape
    qc = qd.clone().requires_grad_(True)
    _composition(qc, b, t, h)[0].backward(dd)
    errs = []
    for (name, got), (_, comp), (_, want) in zip(_thirds(dqkv.cpu()), _thirds(qc.grad.cpu()), _thirds(dref)):
        if t == 1 and name != "dV":
            assert not bool(got.any()) and not bool(want.any())
            continue
        if t == 1:
            assert torch.equal(got, dout)                   # softmax over one key is the constant 1: dout passes to v unchanged
        e = rel_err(got, want)
        errs.append(e)
        print("MEASURED vit attention dk32 bwd", form, (b, t, h), name, "kernel %.3e  torch composition %.3e" % (e, rel_err(comp, want)))
    assert max(errs) < BWD_GATE[form], errs


@pytest.mark.parametrize("b,t,h", SHAPES)
@pytest.mark.parametrize("form", FORMS)
def test_backward_is_deterministic_and_writes_everything(form, b, t, h):
    qkv, dout, _, _, _ = _case(form, b, t, h)
    qd, dd = qkv.to(DEV), dout.to(DEV)
    _, lse = _ops().vit_attention_dk32_fwd_lse(qd, b, t, h)
    first = torch.full_like(qd, float("nan"))
    second = torch.full_like(qd, float("nan"))
    assert _ops().vit_attention_dk32_bwd(qd, dd, lse, b, t, h, out=first) is first
    _ops().vit_attention_dk32_bwd(qd, dd, lse, b, t, h, out=second)
    assert not bool(torch.isnan(first).any())
    assert torch.equal(first, second)
    if t == 1:
        d = h * DK
        assert not bool(first[:, :2 * d].any()) and torch.equal(first[:, 2 * d:], dd)


@pytest.mark.parametrize("form", FORMS)
def test_both_kernels_stay_inside_their_buffers(form):
    b, t, h = 2, 37, 2
    qkv, dout, _, _, _ = _case(form, b, t, h)
    pad = 256                                               # elements: keeps the carved tensors 16-byte aligned

    def carve(src):
        buf = torch.full((src.numel() + 2 * pad,), float("nan"), dtype=src.dtype, device=DEV)
        view = buf[pad:pad + src.numel()].view(src.shape)
        view.copy_(src)
        return buf, view

    ops = _ops()
    qbuf, qd = carve(qkv)
    dbuf, dd = carve(dout)
    out_plain, lse = ops.vit_attention_dk32_fwd_lse(qkv.to(DEV), b, t, h)
    out_carved, lse_carved = ops.vit_attention_dk32_fwd_lse(qd, b, t, h)
    assert torch.equal(out_carved, out_plain) and torch.equal(lse_carved, lse)
    lbuf, ld = carve(lse)
    obuf, od = carve(torch.zeros_like(qkv))
    od.fill_(float("nan"))
    ops.vit_attention_dk32_bwd(qd, dd, ld, b, t, h, out=od)
    want = ops.vit_attention_dk32_bwd(qkv.to(DEV), dout.to(DEV), lse, b, t, h)
    assert torch.equal(od, want)
    for buf in (qbuf, dbuf, lbuf, obuf):
        assert bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[-pad:]).all())
    assert torch.equal(qd, qkv.to(DEV)) and torch.equal(dd, dout.to(DEV))       # inputs untouched


@pytest.mark.parametrize("form", FORMS)
def test_refuses_what_it_does_not_serve(form):
    ops = _ops()
    dt = torch.float32 if form == "x3" else BF

    def operands(b, t, h, dk, shift=0):
        n = b * t * 3 * h * dk
        qkv = torch.zeros(n + 8, dtype=dt, device=DEV)[shift:shift + n].view(b * t, 3 * h * dk)
        return qkv, torch.zeros(b * t, h * dk, dtype=dt, device=DEV), torch.zeros(b, h, t, dtype=torch.float32, device=DEV)

    qkv, dout, lse = operands(1, 256, 1, 32)                # the edge of the domain is served
    assert ops.vit_attention_dk32_supported(256, 32)
    assert ops.vit_attention_dk32_fwd_lse(qkv, 1, 256, 1)[0].shape == (256, 32)
    assert ops.vit_attention_dk32_bwd(qkv, dout, lse, 1, 256, 1).shape == (256, 96)
    for kw, supported in ((dict(t=257, dk=32), False), (dict(t=8, dk=64), False), (dict(t=8, dk=16), False), (dict(t=8, dk=32, shift=1), True)):
        assert ops.vit_attention_dk32_supported(kw["t"], kw["dk"]) is supported
        qkv, dout, lse = operands(1, kw["t"], 2, kw["dk"], kw.get("shift", 0))
        with pytest.raises(ops._ffi.SnuffyHipError, match=r"code -3\): snf_vit_attention_dk32_fwd_lse: unsupported"):
            ops.vit_attention_dk32_fwd_lse(qkv, 1, kw["t"], 2)
        with pytest.raises(ops._ffi.SnuffyHipError, match=r"code -3\): snf_vit_attention_dk32_bwd: unsupported"):
            ops.vit_attention_dk32_bwd(qkv, dout, lse, 1, kw["t"], 2)
    with pytest.raises(ops._ffi.SnuffyHipError, match="GPU tensor"):
        ops.vit_attention_dk32_bwd(torch.zeros(8, 96), torch.zeros(8, 32), torch.zeros(1, 1, 8), 1, 8, 1)
    with pytest.raises(ops._ffi.SnuffyHipError, match="GPU tensor"):
        ops.vit_attention_dk32_fwd_lse(torch.zeros(8, 96), 1, 8, 1)


# ---- autograd layer ----------------------------------------------------------------------------------------------------------------------
def _count(monkeypatch, name):
    """Wrap ops.<name> (a backward entry point) in a recorder of its (qkv shape, heads) -> the list."""
    ops = _ops()
    calls, real = [], getattr(ops, name)

    def wrapped(qkv, *args, **kw):
        calls.append((tuple(qkv.shape), args[4]))
        return real(qkv, *args, **kw)

    monkeypatch.setattr(ops, name, wrapped)
    return calls


def _attn(d, h, seed):
    from snuffy_amd import vit
    torch.manual_seed(seed)
    return vit.Attention(d, num_heads=h, qkv_bias=True).to(DEV)


def test_mae_step_runs_its_decoder_on_the_dk32_kernels(monkeypatch):
    S = _ssl()
    torch.manual_seed(12)
    model = S.MAEPretrainModel(img_size=64, patch_size=16, embed_dim=128, depth=2, num_heads=2, decoder_embed_dim=64, decoder_depth=1,
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
    old, new = _count(monkeypatch, "vit_attention_bwd"), _count(monkeypatch, "vit_attention_dk32_bwd")
    monkeypatch.setattr(S, "FUSED_ATTENTION", True)
    res = {}
    for flag in (True, False):
        monkeypatch.setattr(S, "FUSED_ATTENTION_DK32", flag)
        del old[:], new[:]
        model.zero_grad(set_to_none=True)
        loss, _, _ = model(imgs, 0.75, noise)
        loss.backward()
        res[flag] = (float(loss.detach()), {n: p.grad.clone() for n, p in model.named_parameters() if "adaptmlp" in n and p.grad is not None})
        # the two encoder blocks (dk = 64, T = 1 + 4 kept patches) on the 64-wide kernel in both legs; the decoder block (dk = 32,
        # T = 1 + 16) on the 32-wide one with the switch on and on neither with it off
        assert old == [((4 * 5, 3 * 128), 2)] * 2, (flag, old)
        assert new == ([((4 * 17, 3 * 64), 2)] if flag else []), (flag, new)
    assert abs(res[True][0] - res[False][0]) < 1e-5
    assert len(res[True][1]) >= 12
    for n, on in res[True][1].items():
        e = rel_err(on, res[False][1][n])
        print("MEASURED vit attention dk32 mae on vs off", n, "%.3e" % e)
        assert e < 2e-4, n


def test_saved_state_is_qkv_and_one_float_per_row(monkeypatch):
    S = _ssl()
    b, t, h, d = 2, 197, 16, 512
    attn = _attn(d, h, 2)
    x = torch.randn(b, t, d, device=DEV, generator=torch.Generator(DEV).manual_seed(3), requires_grad=True)
    saved = []

    def run(fn):
        del saved[:]
        with torch.autograd.graph.saved_tensors_hooks(lambda ten: (saved.append(ten), ten)[1], lambda ten: ten):
            return fn()

    qkv = F.linear(x, attn.qkv.weight, attn.qkv.bias).view(b * t, 3 * d)
    out = run(lambda: S.ViTAttentionFn.apply(qkv, b, t, h, attn.scale))
    assert len(saved) == 2
    assert saved[0].data_ptr() == qkv.data_ptr() and saved[0].shape == qkv.shape
    assert saved[1].dtype == torch.float32 and saved[1].numel() == b * h * t
    out.sum().backward()
    assert x.grad is not None and bool(torch.isfinite(x.grad).all())
    for flag, expect in ((True, False), (False, True)):
        monkeypatch.setattr(S, "FUSED_ATTENTION_DK32", flag)
        run(lambda: S._attention(attn, x))
        assert any(ten.numel() == b * h * t * t for ten in saved) is expect, (flag, [tuple(ten.shape) for ten in saved])


def test_autocast_runs_the_bf16_kernels(monkeypatch):
    """The form follows the dtype of the qkv Linear's output: under torch.autocast(bfloat16) both kernels get bf16 tensors."""
    S, ops = _ssl(), _ops()
    b, t, h = 2, 37, 2
    attn = _attn(64, h, 4)
    seen = []
    real_f, real_b = ops.vit_attention_dk32_fwd_lse, ops.vit_attention_dk32_bwd
    monkeypatch.setattr(ops, "vit_attention_dk32_fwd_lse", lambda qkv, *a, **k: (seen.append(("fwd", qkv.dtype)), real_f(qkv, *a, **k))[1])
    monkeypatch.setattr(ops, "vit_attention_dk32_bwd",
                        lambda qkv, dout, *a, **k: (seen.append(("bwd", qkv.dtype, dout.dtype)), real_b(qkv, dout, *a, **k))[1])
    monkeypatch.setattr(S, "FUSED_ATTENTION_DK32", True)
    x = torch.randn(b, t, 64, device=DEV, generator=torch.Generator(DEV).manual_seed(9), requires_grad=True)
    with torch.autocast("cuda", BF):
        y = S._attention(attn, x)
    y.float().sum().backward()
    assert seen == [("fwd", BF), ("bwd", BF, BF)]
    assert y.dtype == BF and x.grad.dtype == torch.float32 and bool(torch.isfinite(x.grad).all()) and bool(x.grad.any())
