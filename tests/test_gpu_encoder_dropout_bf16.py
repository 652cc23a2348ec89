"""Encoder dropout (reference snuffy.py:108, 225, 110) inside the fused bf16 training chain: the masks the new kernels regenerate are
the Philox mask tensor bit for bit, and EncoderLayer0Bf16Fn computes what a plain-torch restatement of the layer computes with the mask
tensors of layer.last_dropout_states, within the bounds of test_fused_bf16_layer0_training_matches_generic_and_fp32."""
import math

import numpy as np
import pytest
import torch

from tests.helpers import BF, DEV, _ops, _parity, _perturbed_state_dict, _run

pytestmark = pytest.mark.gpu
STATE = (0.1, 2 ** 63 + 12345, 2 ** 61 + 77)


def _mask(m, c, state=STATE):
    return _ops().dropout_mask(1, m, c, state[0], state[1], state[2], DEV)[0]


# ---------------------------------------------------------------------------------------------------------------- 1. in-place pass
@pytest.mark.parametrize("m,n,pitch", [(300, 288, 288), (1, 8, 8), (33, 8192, 8192), (512, 3072, 3200)])
def test_in_place_pass_is_the_rounded_product_with_the_mask_tensor(m, n, pitch):
    """snf_dropout_rows_bf16: rows not a multiple of the wave count / width not a multiple of 64; one group; the widest row; a row-pitched
    view of a wider buffer, whose columns beyond n stay as they were."""
    ops = _ops()
    g = torch.Generator().manual_seed(m + n)
    buf = torch.randn(m, pitch, generator=g).to(DEV).to(BF)
    before = buf.clone()
    x = buf[:, :n]
    want = (x.float() * _mask(m, n)).to(BF)
    got = ops.dropout_rows_bf16_(x, STATE)
    assert got.data_ptr() == buf.data_ptr()
    assert torch.equal(buf[:, :n], want)
    assert torch.equal(buf[:, n:], before[:, n:])
    if m > 1:
        kept = float((want != 0).double().mean())
        assert abs(kept - 0.9) < 0.02, kept                              # a mask, not zeros or ones
    ops.dropout_rows_bf16_(x, (0.0, 1, 2))                               # p = 0: nothing changes
    assert torch.equal(buf[:, :n], want)


# ---------------------------------------------------------------------------------------------------------------- 2. own-GEMM form
@pytest.mark.parametrize("m,n,k", [(300, 288, 64), (512, 512, 96)])
def test_gemm_epilogue_masks_the_fp32_value_before_the_one_rounding(m, n, k):
    """snf_gemm_bf16_dropout: zeros exactly where the mask is zero or the ReLU is closed; kept elements within one bf16 ulp of
    bf16(f32 result * scale), the f32 result from snf_gemm_bf16's fp32-output form."""
    ops = _ops()
    g = torch.Generator().manual_seed(m + n + k)
    a = torch.randn(m, k, generator=g).to(DEV).to(BF)
    w = (torch.randn(n, k, generator=g) / math.sqrt(k)).to(DEV).to(BF)
    bias = torch.randn(n, generator=g).to(DEV)
    f32 = ops.gemm_bf16(a, w, bias, "relu", out_dtype=torch.float32)
    mask = _mask(m, n)
    got = ops.gemm_bf16_dropout(a, w, bias, STATE)
    assert got.dtype == BF and tuple(got.shape) == (m, n)
    assert torch.equal(got == 0, (mask == 0) | (f32 == 0))
    want = (f32 * mask).to(BF)
    ulps = (got.view(torch.int16).int() - want.view(torch.int16).int()).abs()      # all values >= 0: the bit patterns are ordered
    print("gemm_bf16_dropout %s: max ulp distance %d, differing %d of %d" % ((m, n, k), int(ulps.max()), int((ulps > 0).sum()), m * n))
    assert int(ulps.max()) <= 1
    open_frac = float(((f32 > 0) & (mask > 0)).double().mean())
    assert 0.3 < open_frac < 0.6, open_frac
    # p = 0 through the same entry point is the plain launch
    assert torch.equal(ops.gemm_bf16_dropout(a, w, bias, (0.0, 1, 2)), ops.gemm_bf16(a, w, bias, "relu"))
    # the routed form: both legs give the same zeros
    for native in (True, False):
        r = ops.linear_bf16_dropout(a, w, bias, None, STATE, prefer_native=native)
        plain = ops.linear_bf16(a, w, bias, None, "relu", prefer_native=native)
        assert torch.equal(r == 0, (mask == 0) | (plain == 0))
        if not native:
            assert torch.equal(r, (plain.float() * mask).to(BF))


def test_gemm_forms_that_do_not_exist_are_errors():
    ops = _ops()
    a = torch.randn(256, 64, device=DEV).to(BF)
    w = torch.randn(256, 64, device=DEV).to(BF)
    bias = torch.zeros(256, device=DEV)
    for kw in (dict(act="none"), dict(act="gelu"), dict(out_dtype=torch.float32)):
        with pytest.raises(ValueError):
            ops.gemm_bf16_dropout(a, w, bias, STATE, **kw)
    lib = ops._ffi.load()
    for act, odt, out in (("gelu", ops.DT_BF16, torch.empty(256, 256, dtype=BF, device=DEV)),
                          ("relu", ops.DT_F32, torch.empty(256, 256, dtype=torch.float32, device=DEV)),
                          ("relu", ops.DT_BF16_HL, torch.empty(256, 512, dtype=BF, device=DEV))):
        rc = lib.snf_gemm_bf16_dropout(ops._p(a), 64, ops._p(w), 64, ops._p(bias), 256, 256, 64, ops.ACT_CODES[act], ops._p(out),
                                       out.stride(0), odt, 0, 0.1, 1, 2, ops._stream())
        assert rc != 0          # a missing kernel is an error, never another kernel
        with pytest.raises(ops._ffi.SnuffyHipError):
            ops.check(rc, "snf_gemm_bf16_dropout")


# ---------------------------------------------------------------------------------------------------------------- 3. assemble
@pytest.mark.parametrize("n,d,k", [(300, 288, 17), (2051, 768, 200)])
def test_assemble_is_the_four_rounded_steps(n, d, k):
    """snf_residual_assemble_dropout_f32: t = zb + b2; t = t * m; z = x + t; z = z + delta[slot], every step rounded on its own."""
    from snuffy_amd import functional as SF
    ops = _ops()
    g = torch.Generator().manual_seed(n + d)
    x = torch.randn(n, d, generator=g).to(DEV)
    zb = torch.randn(n, d, generator=g).to(DEV).to(BF)
    b2 = torch.randn(d, generator=g).to(DEV)
    delta = torch.randn(k, d, generator=g).to(DEV)
    sel = torch.randperm(n, generator=g)[:k].to(DEV)
    slot = ops.slot_map(sel, n)
    t = zb.float() + b2
    t = t * _mask(n, d)
    want = x + t
    want[sel] = want[sel] + delta
    got = ops.residual_assemble_dropout(x, zb, b2, slot, delta, STATE)
    assert torch.equal(got, want)
    assert not torch.equal(got, x + (zb.float() + b2))                  # the mask did something
    # p = 0: what functional.materialize returns for the same Parts
    plain = SF.materialize(SF.Parts(x, add_bf16=zb, add_bias=b2, slot=slot, delta=delta))
    assert torch.equal(ops.residual_assemble_dropout(x, zb, b2, slot, delta, (0.0, 1, 2)), plain)


# ---------------------------------------------------------------------------------------------------------------- 4. colsum_fused(dropout=)
@pytest.mark.parametrize("n,d", [(300, 288), (33, 8192), (512, 3072)])
def test_colsum_fused_with_dropout(n, d):
    """snf_colsum_fused_dropout: the bf16 copy is bf16(dz o mask); the sums are those of the rounded copy (bound of test_colsum_fused_kernel)."""
    ops = _ops()
    g = torch.Generator().manual_seed(n + d)
    dz = torch.randn(n, d, generator=g).to(DEV)
    want = (dz * _mask(n, d)).to(BF)
    s, c = ops.colsum_fused(dz, want_bf16=True, dropout=STATE)
    ref = want.double().sum(0)
    err, tol = (s.double() - ref).abs().max().item(), 2e-5 * max(1.0, ref.abs().max().item()) * (n ** 0.5)
    print("colsum_fused dropout %s: sum error %.3e (bound %.3e)" % ((n, d), err, tol))
    assert torch.equal(c, want)
    assert err <= tol
    s0, c0 = ops.colsum_fused(dz, want_bf16=True, dropout=(0.0, 1, 2))  # p = 0 is the plain pass
    s1, c1 = ops.colsum_fused(dz, want_bf16=True)
    assert torch.equal(c0, c1) and torch.equal(s0, s1)
    with pytest.raises(ValueError):
        ops.colsum_fused(dz, gate=c, dropout=STATE)


# ---------------------------------------------------------------------------------------------------------------- 5. - 7. chain parity
@pytest.mark.parametrize("n,d,h,lam", [(700, 256, 4, 50), (2048, 768, 6, 200), (2051, 768, 6, 200)])
def test_fused_bf16_chain_with_encoder_dropout_matches_the_restated_layer(n, d, h, lam, monkeypatch):
    _parity(monkeypatch, n, d, h, lam)


def test_one_site_alone(monkeypatch):
    """Only feed_forward.dropout.p = 0.2: the chain takes the layer, A and Z draw nothing, parity as above."""
    _parity(monkeypatch, 700, 256, 4, 50, sites=(0.0, 0.2, 0.0))


def test_without_encoder_dropout_the_switch_changes_nothing(monkeypatch):
    """encoder_dropout = 0 in train mode: logits and gradients are torch.equal with FUSED_BF16_ENCODER_DROPOUT on and off, and the same
    number of dropout states is drawn."""
    from snuffy_amd import autograd as SA
    n, d, h, lam = 2048, 768, 6, 200
    sd = _perturbed_state_dict(n, d, h, lam)
    x = torch.randn(1, n, d, device=DEV)
    draws = []
    real_draw = SA.draw_dropout_state
    monkeypatch.setattr(SA, "draw_dropout_state", lambda: (draws.append(1), real_draw())[1])
    calls = []
    real_apply = SA.EncoderLayer0Bf16Fn.apply
    monkeypatch.setattr(SA.EncoderLayer0Bf16Fn, "apply", lambda *a: (calls.append(1), real_apply(*a))[1])
    res = {}
    for switch in (True, False):
        monkeypatch.setattr(SA, "FUSED_BF16_ENCODER_DROPOUT", switch)
        del draws[:]
        _, grads, logits = _run(monkeypatch, sd, x, d, h, lam, "bf16", 0.0)
        res[switch] = (logits, grads, len(draws))
    assert len(calls) == 2
    assert res[True][2] == res[False][2] == 1                            # the attention's own draw
    assert torch.equal(res[True][0], res[False][0])
    for k in res[True][1]:
        assert torch.equal(res[True][1][k], res[False][1][k]), k


# ---------------------------------------------------------------------------------------------------------------- 8. trainer path
def test_trainer_step_with_encoder_dropout_reaches_the_fused_bf16_chain(monkeypatch):
    """One epoch of two synthetic bags through train.Snuffy with --encoder_dropout 0.1 --precision bf16: every step runs
    EncoderLayer0Bf16Fn (and the one-pass critic that goes with it), the losses are finite."""
    from snuffy_amd import autograd as SA
    from snuffy_amd.train import Snuffy, get_args_parser
    torch.manual_seed(0)
    np.random.seed(0)
    a = get_args_parser().parse_args(["--encoder_dropout", "0.1", "--precision", "bf16"])
    a.feats_size, a.num_heads, a.big_lambda, a.optimizer, a.num_epochs = 768, 6, 200, "adamw", 1
    tr = Snuffy(a)
    layer = tr.milnet.b_classifier.encoder.layers[0]
    assert layer.sublayer[0].dropout.p == 0.1 and layer.sublayer[1].dropout.p == 0.1 and layer.feed_forward.dropout.p == 0.1
    calls, offers = [], []
    real_apply = SA.EncoderLayer0Bf16Fn.apply
    monkeypatch.setattr(SA.EncoderLayer0Bf16Fn, "apply", lambda *args: (calls.append(1), real_apply(*args))[1])
    real_critic = SA.critic_train
    monkeypatch.setattr(SA, "critic_train", lambda *args, **kw: (offers.append(1), real_critic(*args, **kw))[1])
    g = np.random.RandomState(3)
    feats = [g.randn(2048, 768).astype(np.float32), g.randn(2051, 768).astype(np.float32)]
    feats[1][:50] += 1.0
    labels = [np.array([0.0], dtype=np.float32), np.array([1.0], dtype=np.float32)]
    res = tr.train((labels, feats, None, None), 1)
    assert len(calls) == 2 and len(offers) == 2
    assert np.isfinite(res["epoch_train_loss"])
    assert all(bool(torch.isfinite(p).all()) for p in tr.milnet.parameters())
    st = layer.last_dropout_states
    assert all(st[s] is not None and st[s][0] == 0.1 for s in ("attn", "A", "H", "Z"))
