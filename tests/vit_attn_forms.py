"""The forms of the differentiable ViT self-attention (ops.VIT_TRAIN_FORMS: `short` dk = 64, T <= 256; `long` dk = 64, 256 < T <= 4096;
`dk32` dk = 32, T <= 256), as the tests and tools/vit_attn_train_time.py see them: one record per form, the helpers, and the bodies of
the tests the forms share.  The host suite (test_vit_attn_forms_host.py) is written once over the table, each test listing its rows.
The GPU files stay one per form (test_gpu_vit_attn_train.py, _long.py, _dk32.py) so that their 190 case ids stay: each names its record
as ROW, keeps the tests that are its own, and calls the shared bodies (`check_*` below) with ROW.  A record carries what the forms differ in as
literal values: ops and switch names, C entry points, shape lists, gates, the rows of the refusal test, the shapes of the autograd-layer
tests, the lines the tests print and the register-scan table.  Every shared body is written once; an assertion one form has and another
lacks stays under an explicit row list inside it.  A new form is one more record, a GPU file of one-line tests and whatever tests are
its own.

Gates are literals, never computed from dk.  Anything cached across tests is keyed on the row as well as the shape.

Measured on an MI355X, largest over each table, and the gates chosen from it (profiles/vit_attn_train.txt, vit_attn_long_train.txt and
vit_attn_dk32_train.txt have every figure):
  short  lse |err| vs float64   fp32 class 5.2e-5 (the x3 scores' own error at |scale s| ~ 11) -> 4 x is above the cap: gate 1e-4;
                                bf16 1.3e-6 -> 4 x, one digit: 6e-6 (cap 5e-2)
         dQ / dK / dV rel_err   fp32 class 2.1e-5 -> 4 x, one digit: 9e-5 (cap 2e-4);  bf16 6.6e-3 -> 2 x, one digit: 2e-2 (cap 3e-2)
         the torch composition of the same dtype on the same inputs: fp32 2.2e-7 ... 1.4e-6, bf16 4.0e-3 ... 1.1e-2
  long   dQ / dK / dV rel_err   fp32 class 2.4e-5 (dQ at (1, 2049, 1); 2.3e-5 at (2, 512, 1), 1.3e-5 at the recipe's (2, 785, 2): no
                                clear growth with T) -> 4 x, one digit: 1e-4 (cap 2e-4);  bf16 4.2e-3 -> 2 x, one digit: 9e-3 (cap 3e-2)
         the torch composition: fp32 5.7e-7 ... 2.3e-6, bf16 5.5e-3 ... 1.6e-2
         block_autograd on against off (D = 128, h = 2, T = 257 and 785): <= 1.9e-6 (gate 2e-4, the short form's)
  dk32   lse |err| vs float64   fp32 class 5.1e-5 -> 4 x is above the cap, so the gate is the cap: 1e-4.  The figure is the x3 scores'
                                own error, not the kernel's: q and k are each hi + lo with lo rounded to bf16 and lo lo dropped (about
                                2^-17 relative per operand), and scale * sum |q_i k_i| is about 8 at these operands, so 6e-5 is what
                                the arithmetic allows; the 64-wide pair measures 5.2e-5 on the same distribution.
                                bf16 1.22e-6 -> 2 x = 2.4e-6, one digit up: 3e-6 (cap 5e-2)
         dQ / dK / dV rel_err   fp32 class 3.1e-5 -> 4 x = 1.24e-4, one digit up: 2e-4 (the cap);  bf16 5.6e-3 -> 2 x = 1.1e-2, one
                                digit up: 2e-2 (cap 3e-2)
         out rel_err            fp32 class 1.64e-5 (torch fp32 composition 9.8e-7) -> 4 x the larger = 6.6e-5, one digit up: 7e-5
                                bf16 3.5e-3 (torch bf16 composition 1.86e-2) -> 2 x the larger = 3.7e-2, one digit up: 4e-2
         the torch composition, backward: fp32 2.6e-7 ... 8.9e-7, bf16 5.0e-3 ... 2.0e-2
"""
import functools
import os
import sys
import types

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import BF, DEV, _ops, rel_err, vit_block_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))                                 # scan_spills

ARITHMETICS = ("x3", "bf16")


def _row(**kw):
    return types.SimpleNamespace(**kw)


SHORT = _row(
    name="short", dk=64, fwd="vit_attention_fwd_lse", bwd="vit_attention_bwd", supported="vit_attention_bwd_supported",
    switch="FUSED_ATTENTION", c_fwd="snf_vit_attention_fwd_lse", c_bwd="snf_vit_attention_bwd",
    shapes=[(1, 1, 1), (2, 17, 1), (2, 32, 2), (2, 33, 1), (2, 37, 2), (3, 50, 3), (2, 197, 6), (2, 224, 2), (2, 225, 2), (2, 256, 2)],
    fwd_only=[(2, 785, 2), (1, 257, 2)],                        # the chunked forms emit lse too
    lse_gate={"x3": 1e-4, "bf16": 6e-6},                        # absolute; caps: 1e-4 / 5e-2
    bwd_gate={"x3": 9e-5, "bf16": 2e-2},                        # tests.helpers.rel_err; caps: 2e-4 / 3e-2
    onoff_gate=2e-4, loss_gate=1e-5,
    carve=[(2, 37, 2)],
    # refusals: the (b, t, h) at the edge of the domain that is served, the (t, dk) the predicate must admit, then (t, dk, pointer
    # shift, what the predicate says): a pointer is not a shape, so the last row is refused by the entry point alone
    edge=(1, 256, 1), admits=[(256, 64)], shift_unit="elements",
    refusals=[(257, 64, 0, False), (8, 32, 0, False), (8, 64, 1, True)],
    fwd_shares_the_domain=False, cpu_t=8, cpu_refusals=("bwd", "fwd"),
    # routing on the host: the (b, t, d) of the input and the heads -- a shape the form serves on the GPU -- and switches held on
    host=_row(x=(2, 37, 128), h=2, hold=()),
    # autograd layer: (b, t, h, d) and the module the attention comes from
    saved=_row(dims=(2, 197, 6, 384), module="block", bott=64, seed=0),
    autocast=_row(dims=(2, 37, 2, 128), module="block", bott=8, seed=0),
    blocks=[(2, 197, 384, 6, 64)], block_idle=(),               # (b, t, d, h, bottleneck); backward wrappers that must stay idle
    # the MAE step: decoder width (2 heads), switches held on, and per recorded wrapper its calls with the switch on and off.  The
    # two encoder blocks are dk = 64 at T = 1 + 4 kept patches; this decoder is dk = 16, which no form serves
    mae=_row(decoder=32, hold=(), calls={"vit_attention_bwd": {True: [((4 * 5, 3 * 128), 2)] * 2, False: []}}),
    say=_row(bwd="vit attention bwd", block="vit attention block on vs off", mae="vit attention mae on vs off"),
    # backward: 4 key-block counts x 2 arithmetics; forward (the lse store is a nullable pointer of the same instantiations): 5 + 4
    kernels={"vit_attention_bwd_kernel<": 8, "vit_attention_bwd_t1_kernel<": 2, "vit_attention_mfma_kernel<": 9}, no_spilled=False,
)
LONG = _row(
    name="long", dk=64, fwd="vit_attention_fwd_lse", bwd="vit_attention_bwd_long", supported="vit_attention_bwd_long_supported",
    switch="FUSED_ATTENTION_LONG", c_fwd="snf_vit_attention_fwd_lse", c_bwd="snf_vit_attention_bwd_long",
    # one key in the second chunk with seven idle waves; one full tile in the second chunk; around exactly two chunks; the patch-8
    # recipe (25 tiles, 4 chunks, batch stride); the forward suite's longest; nine chunks with one row in the last
    shapes=[(2, 257, 1), (1, 288, 2), (1, 511, 1), (2, 512, 1), (1, 513, 2), (2, 785, 2), (1, 1030, 1), (1, 2049, 1)],
    fwd_only=[],
    bwd_gate={"x3": 1e-4, "bf16": 9e-3},                        # tests.helpers.rel_err; caps: 2e-4 / 3e-2
    onoff_gate=2e-4,
    carve=[(2, 257, 1), (1, 513, 2)],
    edge=(1, 257, 1), admits=[(257, 64), (4096, 64)], shift_unit="bytes",
    refusals=[(256, 64, 0, False), (4097, 64, 0, False), (300, 32, 0, False), (300, 64, 4, True)],
    fwd_shares_the_domain=False, cpu_t=300, cpu_refusals=("bwd",),
    host=_row(x=(1, 300, 128), h=2, hold=("FUSED_ATTENTION",)),
    saved=_row(dims=(1, 257, 2, 128), module="block", bott=8, seed=0),
    autocast=_row(dims=(1, 257, 2, 128), module="block", bott=8, seed=0),
    blocks=[(1, 257, 128, 2, 8), (1, 785, 128, 2, 8)], block_idle=("vit_attention_bwd",),
    say=_row(bwd="vit attention bwd long", block="vit attention long block on vs off {t}"),
    kernels={"vit_attention_bwd_dq_kernel<": 2, "vit_attention_bwd_dkv_kernel<": 2}, no_spilled=False,    # one per arithmetic
)
DK32 = _row(
    name="dk32", dk=32, fwd="vit_attention_dk32_fwd_lse", bwd="vit_attention_dk32_bwd", supported="vit_attention_dk32_supported",
    switch="FUSED_ATTENTION_DK32", c_fwd="snf_vit_attention_dk32_fwd_lse", c_bwd="snf_vit_attention_dk32_bwd",
    # the copy kernel; under one tile; the tile edge and an odd head count; ragged tiles; NKB = 4 (100); the decoder's own T and h;
    # the last key block whole, one past it, and the edge of the domain
    shapes=[(1, 1, 1), (2, 17, 1), (2, 32, 2), (2, 33, 3), (2, 37, 2), (3, 50, 3), (1, 100, 2), (1, 197, 16), (2, 224, 2), (2, 225, 2),
            (2, 256, 2)],
    fwd_only=[],
    lse_gate={"x3": 1e-4, "bf16": 3e-6},                        # absolute; caps of the 64-wide pair: 1e-4 / 5e-2
    bwd_gate={"x3": 2e-4, "bf16": 2e-2},                        # tests.helpers.rel_err; caps of the 64-wide pair: 2e-4 / 3e-2
    out_gate={"x3": 7e-5, "bf16": 4e-2},                        # tests.helpers.rel_err; 4 x / 2 x the larger of kernel and torch composition
    onoff_gate=2e-4, loss_gate=1e-5,
    carve=[(2, 37, 2)],
    edge=(1, 256, 1), admits=[(256, 32)], shift_unit="elements",
    refusals=[(257, 32, 0, False), (8, 64, 0, False), (8, 16, 0, False), (8, 32, 1, True)],
    fwd_shares_the_domain=True, cpu_t=8, cpu_refusals=("bwd", "fwd"),
    host=_row(x=(2, 37, 64), h=2, hold=()),
    saved=_row(dims=(2, 197, 16, 512), module="attention", seed=2),
    autocast=_row(dims=(2, 37, 2, 64), module="attention", seed=4),
    # the two encoder blocks on the 64-wide kernel in both legs; the decoder block (dk = 32, T = 1 + 16) on the 32-wide one with the
    # switch on and on neither with it off
    mae=_row(decoder=64, hold=("FUSED_ATTENTION",),
             calls={"vit_attention_bwd": {True: [((4 * 5, 3 * 128), 2)] * 2, False: [((4 * 5, 3 * 128), 2)] * 2},
                    "vit_attention_dk32_bwd": {True: [((4 * 17, 3 * 64), 2)], False: []}}),
    say=_row(bwd="vit attention dk32 bwd", mae="vit attention dk32 mae on vs off"),
    # the key-block counts the dispatch of csrc/vit_attn_dk32.hip builds (2, 4, 8), each in two arithmetics
    kernels={"vit_attn32_fwd_kernel<": 6, "vit_attn32_bwd_kernel<": 6, "vit_attn32_bwd_t1_kernel<": 2}, no_spilled=True,
)
ROWS = (SHORT, LONG, DK32)


def by_row(rows):
    return [pytest.param(row, id=row.name) for row in rows]


def _ssl():
    from snuffy_amd import ssl_pretrain
    return ssl_pretrain


def composition(qkv, b, t, h):
    """The composition of tests/test_gpu_vit.ref_attention, in the dtype of qkv -> (out [b*t, d], scores * scale)."""
    d = qkv.shape[1] // 3
    dk = d // h
    q, k, v = qkv.view(b, t, 3, h, dk).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-2, -1)) * dk ** -0.5
    return (s.softmax(-1) @ v).transpose(1, 2).reshape(b * t, d), s


def operands(dk, form, b, t, h):
    """qkv and dout of a table entry (host tensors in the arithmetic's dtype)."""
    g = torch.Generator().manual_seed(1000 * t + 10 * h + b)
    qkv = torch.randn(b * t, 3 * h * dk, generator=g) * 1.5
    dout = torch.randn(b * t, h * dk, generator=g)
    return (qkv.to(BF), dout.to(BF)) if form == "bf16" else (qkv, dout)


@functools.lru_cache(maxsize=None)
def _case(name, dk, form, b, t, h):
    qkv, dout = operands(dk, form, b, t, h)
    q64 = qkv.double().requires_grad_(True)
    out, s = composition(q64, b, t, h)
    out.backward(dout.double())
    return qkv, dout, out.detach(), torch.logsumexp(s.detach(), -1), q64.grad


def case(row, form, b, t, h):
    """Operands of one table entry and the float64 yardstick computed from those operands on the CPU: qkv, dout, out, lse,
    dQ | dK | dV.  Computed once per (row, entry) and shared; nothing writes to it."""
    return _case(row.name, row.dk, form, b, t, h)


def thirds(dqkv):
    d = dqkv.shape[1] // 3
    return (("dQ", dqkv[:, :d]), ("dK", dqkv[:, d:2 * d]), ("dV", dqkv[:, 2 * d:]))


def carve(src, pad=256):
    """A device copy of `src` between two runs of `pad` NaN elements (256 keeps it 16-byte aligned) -> (the whole buffer, the copy)."""
    buf = torch.full((src.numel() + 2 * pad,), float("nan"), dtype=src.dtype, device=DEV)
    view = buf[pad:pad + src.numel()].view(src.shape)
    view.copy_(src)
    return buf, view


def count(monkeypatch, name):
    """Wrap ops.<name> in a recorder of its (qkv shape, heads) -> the list."""
    ops = _ops()
    calls, real = [], getattr(ops, name)

    def wrapped(qkv, *args, **kw):
        calls.append((tuple(qkv.shape), args[2] if name.endswith("fwd_lse") else args[4]))
        return real(qkv, *args, **kw)

    monkeypatch.setattr(ops, name, wrapped)
    return calls


def vit_model(embed, heads, depth, bott=64, seed=0):
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


def attention_module(spec):
    """The attention of a `saved` / `autocast` record on the device: a block's of `vit_model`, or a bare vit.Attention."""
    _, _, h, d = spec.dims
    if spec.module == "block":
        return vit_model(d, h, 1, bott=spec.bott, seed=spec.seed).blocks[0].attn
    from snuffy_amd import vit
    torch.manual_seed(spec.seed)
    return vit.Attention(d, num_heads=h, qkv_bias=True).to(DEV)


def mae_model(decoder_embed_dim):
    """A two-block MAE-adapter model with a one-block, two-head decoder of that width, nothing at its init value, dropout off."""
    S = _ssl()
    torch.manual_seed(12)
    model = S.MAEPretrainModel(img_size=64, patch_size=16, embed_dim=128, depth=2, num_heads=2, decoder_embed_dim=decoder_embed_dim,
                               decoder_depth=1, decoder_num_heads=2, mlp_ratio=4, norm_layer=functools.partial(torch.nn.LayerNorm, eps=1e-6),
                               norm_pix_loss=True, adapter_ffn_scalar="1.0", adapter_ffn_num=8, adapter_d_model=128)
    g = torch.Generator().manual_seed(13)
    with torch.no_grad():
        for n, p in model.named_parameters():               # nothing at its init value (the LoRA zero init would hide the adapters)
            if p.requires_grad and "adaptmlp" in n:
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    for m in model.modules():
        if isinstance(getattr(m, "dropout", None), float):
            m.dropout = 0.0
    return model.to(DEV).train(), g


# ---- GPU test bodies: written once, called by the one-per-form GPU files with their ROW -------------------------------------------------------
def check_backward_against_float64(row, form, b, t, h):
    ops = _ops()
    qkv, dout, _, _, dref = case(row, form, b, t, h)
    if row in (LONG,):                                      # the yardstick is sane: no third of the reference is zero or non-finite
        for name, want in thirds(dref):
            assert bool(torch.isfinite(want).all()) and float(want.norm()) > 0, name
    qd, dd = qkv.to(DEV), dout.to(DEV)
    _, lse = getattr(ops, row.fwd)(qd, b, t, h)
    dqkv = getattr(ops, row.bwd)(qd, dd, lse, b, t, h)
    assert dqkv.dtype == qkv.dtype and dqkv.shape == qkv.shape
    # the torch composition in the same dtype on the same device: not a yardstick, printed for scale
    qc = qd.clone().requires_grad_(True)
    composition(qc, b, t, h)[0].backward(dd)
    errs = []
    for (name, got), (_, comp), (_, want) in zip(thirds(dqkv.cpu()), thirds(qc.grad.cpu()), thirds(dref)):
        if t == 1 and name != "dV":
            assert not bool(got.any()) and not bool(want.any())
            continue
        if t == 1 and row in (DK32,):
            assert torch.equal(got, dout)                   # softmax over one key is the constant 1: dout passes to v unchanged
        e = rel_err(got, want)
        errs.append(e)
        print("MEASURED", row.say.bwd, form, (b, t, h), name, "kernel %.3e  torch composition %.3e" % (e, rel_err(comp, want)))
    assert max(errs) < row.bwd_gate[form], errs


def check_backward_is_deterministic_and_writes_everything(row, form, b, t, h):
    ops = _ops()
    qkv, dout, _, _, _ = case(row, form, b, t, h)
    qd, dd = qkv.to(DEV), dout.to(DEV)
    _, lse = getattr(ops, row.fwd)(qd, b, t, h)
    first = torch.full_like(qd, float("nan"))
    second = torch.full_like(qd, float("nan"))
    assert getattr(ops, row.bwd)(qd, dd, lse, b, t, h, out=first) is first
    getattr(ops, row.bwd)(qd, dd, lse, b, t, h, out=second)
    assert not bool(torch.isnan(first).any())
    assert torch.equal(first, second)
    if t == 1:      # softmax over one key is the constant 1: nothing flows to q and k, dout passes to v unchanged
        d = h * row.dk
        assert not bool(first[:, :2 * d].any()) and torch.equal(first[:, 2 * d:], dd)


def check_kernels_stay_inside_their_buffers(row, form, b, t, h):
    """Every tensor sits between two runs of NaN: nothing outside is written, and (long) the NaN after each tensor's last row, where
    rows past T of the last chunk would be, reaches no result."""
    ops = _ops()
    fwd, bwd = getattr(ops, row.fwd), getattr(ops, row.bwd)
    qkv, dout, _, _, _ = case(row, form, b, t, h)
    qbuf, qd = carve(qkv)
    dbuf, dd = carve(dout)
    out_plain, lse = fwd(qkv.to(DEV), b, t, h)
    if row in (DK32,):                                      # the forward on the carved operand
        out_carved, lse_carved = fwd(qd, b, t, h)
        assert torch.equal(out_carved, out_plain) and torch.equal(lse_carved, lse)
    lbuf, ld = carve(lse)
    obuf, od = carve(torch.zeros_like(qkv))
    od.fill_(float("nan"))
    bwd(qd, dd, ld, b, t, h, out=od)
    want = bwd(qkv.to(DEV), dout.to(DEV), lse, b, t, h)
    if row in (LONG,):
        assert not bool(torch.isnan(od).any())
    assert torch.equal(od, want)
    for buf in (qbuf, dbuf, lbuf, obuf):
        assert bool(torch.isnan(buf[:256]).all()) and bool(torch.isnan(buf[-256:]).all())
    assert torch.equal(qd, qkv.to(DEV)) and torch.equal(dd, dout.to(DEV))       # inputs untouched
    if row in (LONG,):
        assert torch.equal(ld, lse)


def check_refuses_what_it_does_not_serve(row, form):
    ops = _ops()
    fwd, bwd, supported = getattr(ops, row.fwd), getattr(ops, row.bwd), getattr(ops, row.supported)
    dt = torch.float32 if form == "x3" else BF

    def zeros(b, t, h, dk, shift=0):
        n = b * t * 3 * h * dk
        qkv = torch.zeros(n + 8, dtype=dt, device=DEV)[shift:shift + n].view(b * t, 3 * h * dk)
        return qkv, torch.zeros(b * t, h * dk, dtype=dt, device=DEV), torch.zeros(b, h, t, dtype=torch.float32, device=DEV)

    b, t, h = row.edge                                      # the edge of the domain is served
    qkv, dout, lse = zeros(b, t, h, row.dk)
    assert bwd(qkv, dout, lse, b, t, h).shape == (b * t, 3 * h * row.dk)
    if row.fwd_shares_the_domain:
        assert fwd(qkv, b, t, h)[0].shape == (b * t, h * row.dk)
    for t, dk in row.admits:
        assert supported(t, dk)
    for t, dk, shift, admitted in row.refusals:
        assert supported(t, dk) is admitted
        if row.shift_unit == "bytes":
            shift //= torch.zeros((), dtype=dt).element_size()
        qkv, dout, lse = zeros(1, t, 2, dk, shift)
        with pytest.raises(ops._ffi.SnuffyHipError, match=r"code -3\): %s: unsupported" % row.c_bwd):
            bwd(qkv, dout, lse, 1, t, 2)
        if row.fwd_shares_the_domain:
            with pytest.raises(ops._ffi.SnuffyHipError, match=r"code -3\): %s: unsupported" % row.c_fwd):
                fwd(qkv, 1, t, 2)
    t = row.cpu_t
    with pytest.raises(ops._ffi.SnuffyHipError, match="GPU tensor"):
        bwd(torch.zeros(t, 3 * row.dk), torch.zeros(t, row.dk), torch.zeros(1, 1, t), 1, t, 1)
    if "fwd" in row.cpu_refusals:
        with pytest.raises(ops._ffi.SnuffyHipError, match="GPU tensor"):
            fwd(torch.zeros(t, 3 * row.dk), 1, t, 1)


def check_saved_state_is_qkv_and_one_float_per_row(monkeypatch, row):
    S = _ssl()
    b, t, h, d = row.saved.dims
    attn = attention_module(row.saved)
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
        monkeypatch.setattr(S, row.switch, flag)
        run(lambda: S._attention(attn, x))
        assert any(ten.numel() == b * h * t * t for ten in saved) is expect, (flag, [tuple(ten.shape) for ten in saved])


def check_block_with_the_kernels_matches_the_composition(monkeypatch, row, b, t, d, h, bott):
    S = _ssl()
    blk = vit_model(d, h, 1, bott=bott).blocks[0]
    g = torch.Generator().manual_seed(5)
    x0, dy = torch.randn(b, t, d, generator=g).to(DEV), torch.randn(b, t, d, generator=g).to(DEV)
    calls, idle = count(monkeypatch, row.bwd), [count(monkeypatch, name) for name in row.block_idle]
    res = {}
    for flag in (True, False):
        monkeypatch.setattr(S, row.switch, flag)
        blk.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        y = S.block_autograd(blk, x, True)
        y.backward(dy)
        res[flag] = [("y", y.detach()), ("dx", x.grad)] + [(n, p.grad.clone()) for n, p in blk.adaptmlp.named_parameters() if p.grad is not None and p.numel() > 1]
        assert calls == [((b * t, 3 * d), h)], (flag, calls)                # once with the switch on, not at all with it off
        assert not any(idle)
    assert len(res[True]) == 6                              # output, d/dx, the adapter's two weights and two biases
    for (name, on), (_, off) in zip(res[True], res[False]):
        e = rel_err(on, off)
        print("MEASURED", row.say.block.format(t=t), name, "%.3e" % e)
        assert e < row.onoff_gate, name


def check_mae_step_on_the_kernels(monkeypatch, row):
    S = _ssl()
    model, g = mae_model(row.mae.decoder)
    imgs = torch.rand(4, 3, 64, 64, generator=g).to(DEV)
    noise = torch.rand(4, 16, generator=g).to(DEV)
    recorded = {name: count(monkeypatch, name) for name in row.mae.calls}
    for name in row.mae.hold:
        monkeypatch.setattr(S, name, True)
    res = {}
    for flag in (True, False):
        monkeypatch.setattr(S, row.switch, flag)
        for calls in recorded.values():
            del calls[:]
        model.zero_grad(set_to_none=True)
        loss, _, _ = model(imgs, 0.75, noise)
        loss.backward()
        res[flag] = (float(loss.detach()), {n: p.grad.clone() for n, p in model.named_parameters() if "adaptmlp" in n and p.grad is not None})
        for name, calls in recorded.items():
            assert calls == row.mae.calls[name][flag], (flag, name, calls)
    assert abs(res[True][0] - res[False][0]) < row.loss_gate
    assert len(res[True][1]) >= 12
    for n, on in res[True][1].items():
        e = rel_err(on, res[False][1][n])
        print("MEASURED", row.say.mae, n, "%.3e" % e)
        assert e < row.onoff_gate, n


def check_autocast_runs_the_bf16_kernels(monkeypatch, row):
    """The form follows the dtype of the qkv Linear's output: under torch.autocast(bfloat16) both kernels get bf16 tensors."""
    S, ops = _ssl(), _ops()
    b, t, h, d = row.autocast.dims
    attn = attention_module(row.autocast)
    seen = []
    real_f, real_b = getattr(ops, row.fwd), getattr(ops, row.bwd)
    monkeypatch.setattr(ops, row.fwd, lambda qkv, *a, **k: (seen.append(("fwd", qkv.dtype)), real_f(qkv, *a, **k))[1])
    monkeypatch.setattr(ops, row.bwd, lambda qkv, dout, *a, **k: (seen.append(("bwd", qkv.dtype, dout.dtype)), real_b(qkv, dout, *a, **k))[1])
    monkeypatch.setattr(S, row.switch, True)
    x = torch.randn(b, t, d, device=DEV, generator=torch.Generator(DEV).manual_seed(9), requires_grad=True)
    with torch.autocast("cuda", BF):
        y = S._attention(attn, x)
    y.float().sum().backward()
    assert seen == [("fwd", BF), ("bwd", BF, BF)]
    assert y.dtype == BF and x.grad.dtype == torch.float32 and bool(torch.isfinite(x.grad).all()) and bool(x.grad.any())


# ---- host side ---------------------------------------------------------------------------------------------------------------------------
class Attn(torch.nn.Module):
    """What ssl_pretrain._attention reads of an attention module."""

    def __init__(self, d, h):
        super().__init__()
        self.num_heads, self.scale = h, (d // h) ** -0.5
        self.qkv, self.proj = torch.nn.Linear(d, 3 * d), torch.nn.Linear(d, d)


class OnGpu(torch.Tensor):
    """A CPU tensor that claims the GPU: takes is_cuda out of the routing question."""
    is_cuda = True

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        return super().__torch_function__(func, types, args, kwargs or {})


def scan_registers(row):
    """The register scan of the built objects over `row.kernels` -> ({kernel name: instantiations seen}, [kernels that use scratch --
    or, where the row says so, spilled registers]); skips where there are no build objects."""
    import scan_spills
    objdir = os.path.join(scan_spills.ROOT, "snuffy_amd", "build")
    if not os.path.isdir(objdir) or not any(f.endswith(".o") for f in os.listdir(objdir)):
        pytest.skip("no build objects here (the library was built elsewhere)")
    try:
        ks = scan_spills.kernels(objdir)
    except RuntimeError as exc:
        pytest.skip(str(exc))
    names = scan_spills.demangle([k[1] for k in ks])
    seen = dict.fromkeys(row.kernels, 0)
    bad = []
    for (obj, _, scratch, spilled, _vg), name in zip(ks, names):
        for key in seen:
            if key in name:
                seen[key] += 1
                if scratch or (row.no_spilled and spilled):
                    bad.append((obj, name[:120], scratch, spilled))
    return seen, bad
