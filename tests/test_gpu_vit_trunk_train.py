"""Frozen-trunk training route of adapter pre-training on the GPU (ssl_pretrain.FUSED_TRUNK): the GELU row kernels of
csrc/vit_train.hip, one frozen block with the switch on against off, where the GEMMs land, what steps aside, what is saved, and the
fixture steps F11 / F12.  Tables, operands, references and gates: tests/vit_trunk_forms.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import vit_trunk_forms as V

pytestmark = pytest.mark.gpu
DEV = V.DEV


def _mods():
    from snuffy_amd import ops, ssl_pretrain
    return ops, ssl_pretrain


# ---- the row kernels ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,strided", V.KERNEL_SHAPES)
def test_images_agree_between_formats_and_with_float64(m, n, strided):
    ops, _ = _mods()
    pre, da = V.kernel_operands(m, n, strided)
    for name, run, want, gate in (("gelu", lambda f: ops.gelu_image(pre, f), V.gelu64(pre), V.GELU_GATE),
                                  ("gelu_bwd", lambda f: ops.gelu_bwd_image(da, pre, f), da.double() * V.gelu_slope64(pre), V.GELU_BWD_GATE)):
        halves = {}
        for fmt in ("hl", "cat"):
            img = run(fmt)
            assert img.dtype == torch.bfloat16 and tuple(img.shape) == (m, (2 if fmt == "hl" else 3) * n)
            assert torch.equal(img.view(torch.int16), run(fmt).view(torch.int16))                    # two runs, bit for bit
            halves[fmt] = V.decode(img, fmt, n)
            e = V.rel_err(halves[fmt][0].double() + halves[fmt][1].double(), want)
            print("MEASURED", name, fmt, (m, n), "strided" if strided else "", "%.3e" % e)
            assert e < gate, (name, fmt)
        for a, b in zip(halves["hl"], halves["cat"]):                                               # the same hi and lo values
            assert torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16)), name
        hi, lo = halves["hl"]
        assert bool(torch.isfinite(hi.float()).all()) and bool(torch.isfinite(lo.float()).all())


def test_the_split_is_the_one_of_the_split_kernels():
    """hi = bf16(v), lo = bf16(v - hi): where GELU is the identity in fp32 (x >= 6: erff is 1) the image is split_hl_rows' / split3_rows' own."""
    ops, _ = _mods()
    g = torch.Generator().manual_seed(2)
    x = (6.0 + 30.0 * torch.rand(37, 64, generator=g)).to(DEV)
    assert torch.equal(ops.gelu_image(x, "hl").view(torch.int16), ops.split_hl_rows(x).view(torch.int16))
    assert torch.equal(ops.gelu_image(x, "cat").view(torch.int16), ops.split3_rows(x).view(torch.int16))
    ones = torch.ones_like(x)
    assert torch.equal(ops.gelu_bwd_image(x, 40.0 * ones, "hl").view(torch.int16), ops.split_hl_rows(x).view(torch.int16))
    assert torch.equal(ops.gelu_bwd_image(x, 40.0 * ones, "cat").view(torch.int16), ops.split3_rows(x).view(torch.int16))


@pytest.mark.parametrize("fmt", ["hl", "cat"])
def test_outputs_stay_inside_their_buffers(fmt):
    ops, _ = _mods()
    guard = 64
    for m, n, strided in V.KERNEL_SHAPES:
        pre, da = V.kernel_operands(m, n, strided)
        size = m * n * (2 if fmt == "hl" else 3)
        for run in (lambda out: ops.gelu_image(pre, fmt, out=out), lambda out: ops.gelu_bwd_image(da, pre, fmt, out=out)):
            buf = torch.full((size + 2 * guard,), 0x5a5a, dtype=torch.int16, device=DEV)
            body = buf[guard:guard + size].view(torch.bfloat16).view(m, -1)
            assert run(body) is body
            assert bool((buf[:guard] == 0x5a5a).all()) and bool((buf[guard + size:] == 0x5a5a).all())
            fresh = run(None)
            assert torch.equal(body.view(torch.int16), fresh.view(torch.int16))


def test_shapes_off_the_granule_are_refused():
    ops, _ = _mods()
    x = torch.zeros(4, 48, device=DEV)
    for fn in (lambda f, t: ops.gelu_image(t, f), lambda f, t: ops.gelu_bwd_image(t, t, f)):
        with pytest.raises(ValueError):
            fn("hl", x)                                      # 48 % 32
        fn("cat", x)
        with pytest.raises(ValueError):
            fn("cat", x[:, :36].contiguous())                # 36 % 8
        with pytest.raises(ValueError):
            fn("rows", x)
    with pytest.raises(ValueError):
        ops.gelu_bwd_image(torch.zeros(3, 48, device=DEV), x, "cat")
    with pytest.raises(TypeError):
        ops.gelu_image(x.double(), "cat")


# ---- one frozen block ---------------------------------------------------------------------------------------------------------------------
def _block_on_off(monkeypatch, b, t, d, h, bott, expect):
    ops, S = _mods()
    blk = V.frozen_block(d, h, bott)
    x0, dy = V.block_operands(b, t, d)
    calls = V.count_gemms(monkeypatch, ops)
    res = {}
    for flag in (True, False):
        monkeypatch.setattr(S, "FUSED_TRUNK", flag)
        del calls[:]
        res[flag] = V.run_block(S, blk, x0, dy)
        assert len(calls) == (8 if flag else 0), (flag, calls)
        if flag:
            assert {c[0] for c in calls} == expect, calls
    ref = V.block_float64(S, blk, x0, dy)
    assert len(res[True]) == 6
    for (name, on), (_, off), (_, want) in zip(res[True], res[False], ref):
        e = V.rel_err(on, off)
        print("MEASURED block", (b, t, d, h), name, "on/off %.3e  on/f64 %.3e  off/f64 %.3e" % (e, V.rel_err(on, want), V.rel_err(off, want)))
        assert e < V.ONOFF_GATE, name


@pytest.mark.parametrize("b,t,d,h,bott", V.BLOCK_SHAPES)
def test_frozen_block_matches_the_composition(monkeypatch, b, t, d, h, bott):
    _block_on_off(monkeypatch, b, t, d, h, bott, {"gemm_x3"})


def test_frozen_block_on_both_gemm_forms(monkeypatch):
    ops, _ = _mods()
    t, d, h, bott = V.BLOCK_HL
    _block_on_off(monkeypatch, V.hl_batch(ops, t, d), t, d, h, bott, {"gemm_hl", "gemm_x3"})


# ---- where the work lands -----------------------------------------------------------------------------------------------------------------
def test_every_trunk_projection_lands_on_a_split_gemm(monkeypatch):
    ops, S = _mods()
    monkeypatch.setattr(S, "FUSED_TRUNK", True)
    depth, d = 3, 64
    model = V.freeze_trunk(V.small_model(embed=d, depth=depth)).to(DEV)
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(1)).to(DEV)
    m = 2 * 5
    for n, k in ((3 * d, d), (d, d), (4 * d, d), (d, 4 * d)):
        assert ops.vit_trunk_train_supported(m, n, k) and ops.vit_trunk_train_supported(m, k, n)
    calls = V.count_gemms(monkeypatch, ops)
    linears, applied = [], []
    real_linear = F.linear
    monkeypatch.setattr(F, "linear", lambda *a, **kw: (linears.append(tuple(a[1].shape)), real_linear(*a, **kw))[1])
    for fn in (S.FrozenLinearFn, S.FrozenNormLinearFn, S.FrozenMlpFn):
        monkeypatch.setattr(fn, "apply", lambda *a, _fn=fn, _real=fn.apply: (applied.append(_fn.__name__), _real(*a))[1])
    y = S.vit_forward_autograd(model, x)
    per_block = [(m, 3 * d), (m, d), (m, 4 * d), (m, d)]                                         # qkv, proj, fc1, fc2
    assert [c[1:] for c in calls] == per_block * depth, calls
    assert len(linears) == 2 * depth and all(8 in s for s in linears), linears                   # the adapters' down and up
    assert applied == ["FrozenNormLinearFn", "FrozenLinearFn", "FrozenMlpFn"] * (depth - 1)     # block 0: nothing upstream needs a gradient
    del calls[:]
    y.square().sum().backward()
    assert sorted(c[1:] for c in calls) == sorted([(m, 4 * d), (m, d), (m, d), (m, d)] * (depth - 1)), calls
    assert all(p.grad is not None for n, p in model.named_parameters() if "adaptmlp" in n)
    del calls[:], linears[:], applied[:]
    with torch.no_grad():                                                                        # the teacher
        y = S.vit_forward_autograd(model, x)
    assert [c[1:] for c in calls] == per_block * depth and not applied and y.grad_fn is None and len(linears) == 2 * depth


# ---- stepping aside -----------------------------------------------------------------------------------------------------------------------
def _all_trainable(blk):
    for p in blk.parameters():
        p.requires_grad = True


def _weights_frozen_biases_trainable(blk):
    for n, p in blk.named_parameters():
        p.requires_grad = "adaptmlp" in n or n.endswith(".bias")


@pytest.mark.parametrize("case", ["nothing frozen", "trainable biases", "autocast", "cpu", "switch off"])
def test_the_route_steps_aside(monkeypatch, case):
    ops, S = _mods()
    b, t, d, h, bott = V.BLOCK_SHAPES[0]
    blk = V.frozen_block(d, h, bott)
    x0, dy = V.block_operands(b, t, d)
    if case == "nothing frozen":
        _all_trainable(blk)
    elif case == "trainable biases":
        _weights_frozen_biases_trainable(blk)
    elif case == "cpu":
        blk, x0, dy = blk.cpu(), x0.cpu(), dy.cpu()
    calls = V.count_gemms(monkeypatch, ops)
    res = {}
    for flag in ((False, False) if case == "switch off" else (True, False)):
        monkeypatch.setattr(S, "FUSED_TRUNK", flag)
        if case == "autocast":
            with torch.autocast("cuda", torch.bfloat16):
                res[len(res)] = V.run_block(S, blk, x0, dy)
        else:
            res[len(res)] = V.run_block(S, blk, x0, dy)
    assert not calls
    assert len(res[0]) == 6 and all(torch.equal(a, b) for (_, a), (_, b) in zip(res[0], res[1]))
    assert all(bool(torch.isfinite(a).all()) for _, a in res[0])


# ---- saved state --------------------------------------------------------------------------------------------------------------------------
def test_saved_state(monkeypatch):
    ops, S = _mods()
    monkeypatch.setattr(S, "FUSED_TRUNK", True)
    b, t, d, h, bott = V.BLOCK_SHAPES[1]
    blk = V.frozen_block(d, h, bott)
    m = b * t
    x = torch.randn(b, t, d, device=DEV, generator=torch.Generator(DEV).manual_seed(3), requires_grad=True)
    saved = []

    def run(fn):
        del saved[:]
        with torch.autograd.graph.saved_tensors_hooks(lambda ten: (saved.append(ten), ten)[1], lambda ten: ten):
            return fn()

    def functions(y):
        """Names of the autograd nodes between y and x."""
        names, todo = [], [y.grad_fn]
        while todo:
            f = todo.pop()
            if f is not None:
                names.append(type(f).__name__)
                todo.extend(n for n, _ in f.next_functions)
        return names

    y = run(lambda: S._linear(x, blk.attn.proj))
    assert "FrozenLinearFnBackward" in functions(y) and saved == []
    y.sum().backward()
    assert x.grad is not None and bool(torch.isfinite(x.grad).all())
    y = run(lambda: S._norm_mlp(blk.norm2, blk.mlp, x))
    assert "FrozenMlpFnBackward" in functions(y)
    assert sorted(tuple(ten.shape) for ten in saved) == [(m, d), (m, 4 * d)] and all(ten.dtype == torch.float32 for ten in saved)
    y = run(lambda: S._norm_linear(blk.norm1, blk.attn.qkv, x))
    assert "FrozenNormLinearFnBackward" in functions(y) and [tuple(ten.shape) for ten in saved] == [(m, d)]


# ---- the fixture steps --------------------------------------------------------------------------------------------------------------------
def test_dino_fixture_step_on_the_route(monkeypatch):
    """The DINO step of tests/test_gpu_vit.test_adapter_pretraining_steps_on_the_device with the switch forced on, against fixture F11
    and with that test's own tolerances."""
    from tests import test_ssl_pretrain as T
    ops, S = _mods()
    monkeypatch.setattr(S, "FUSED_TRUNK", True)
    calls = V.count_gemms(monkeypatch, ops)
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
    depth = len(student.backbone.blocks)
    assert len(calls) == 4 * depth                              # one resolution, no backward
    loss = lm(student(crops), t_out, 1)
    loss.backward()
    assert len(calls) == 4 * depth + 2 * (4 * depth + 4 * (depth - 1))     # two resolutions, backward from block 1 on
    print("MEASURED F11 loss", "%.3e" % abs(float(loss.detach()) - float(z["step_loss"])))
    assert abs(float(loss.detach()) - float(z["step_loss"])) < 1e-4
    S.clip_gradients(student, 0.3)
    seen = 0
    for n, p in student.named_parameters():
        if p.grad is not None and "adaptmlp" in n:
            ref = z["grad." + n]
            assert np.allclose(p.grad.cpu().numpy(), ref, rtol=2e-3, atol=1e-3 * np.abs(ref).max() + 1e-7), n
            seen += 1
    assert seen >= 4


def test_mae_fixture_step_on_the_route(monkeypatch):
    """The MAE step of the same test against fixture F12, the trunk frozen (adapters and decoder_pred train), the switch forced on."""
    from tests import test_ssl_pretrain as T
    ops, S = _mods()
    monkeypatch.setattr(S, "FUSED_TRUNK", True)
    calls = V.count_gemms(monkeypatch, ops)
    z = T._npz("f12_mae_pretrain.npz")
    model = T._mae()
    model.load_state_dict(T._sd(z))
    model = model.to(DEV).train()
    for n, p in model.named_parameters():
        p.requires_grad = "adaptmlp" in n or n.startswith("decoder_pred.")
    loss, pred, mask = model(torch.from_numpy(z["imgs"]).to(DEV), 0.75, torch.from_numpy(z["noise"]).to(DEV))
    loss.backward()
    blocks = len(model.blocks) + len(model.decoder_blocks)
    assert len(calls) == 4 * blocks + 4 * (blocks - 1), calls
    print("MEASURED F12 loss", "%.3e" % abs(float(loss.detach()) - float(z["loss"])))
    assert np.array_equal(mask.cpu().numpy(), z["mask"]) and abs(float(loss.detach()) - float(z["loss"])) < 1e-4
    seen = 0
    for n, p in model.named_parameters():
        if p.grad is not None and "grad." + n in z.files:
            ref = z["grad." + n]
            assert np.allclose(p.grad.cpu().numpy(), ref, rtol=2e-3, atol=1e-3 * np.abs(ref).max()), n
            seen += 1
    assert model.decoder_pred.weight.grad is not None and seen >= 1
