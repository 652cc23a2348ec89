"""Encoder dropout (reference snuffy.py:108, 225, 110) inside the fused fp32-class training chain: the masks the GEMM epilogues and the
dz split pass regenerate are the Philox mask tensor bit for bit, and the chain computes what a plain-torch restatement of the layer
computes with those mask tensors."""
import math

import numpy as np
import pytest
import torch

from tests.helpers import DEV, _ops, _perturbed_state_dict, _restated_layer, build_amd_milnet

pytestmark = pytest.mark.gpu


def _operands(m, n, k, seed):
    ops = _ops()
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(m, k, generator=g).to(DEV)
    w = (torch.randn(n, k, generator=g) / math.sqrt(k)).to(DEV)
    bias = torch.randn(n, generator=g).to(DEV)
    return ops.split_hl_rows(a), ops.split_hl_rows(w), bias, g


# tile-aligned; ragged (m not a multiple of 256, n % 32 == 0); a shape whose last round of tiles is split over K
SHAPES_H = [(512, 512, 96), (300, 288, 64)]
SHAPES_Z = [(512, 512, 96), (300, 288, 64), (8348, 2048, 1024)]
STATE = (0.1, 2 ** 63 + 12345, 2 ** 61 + 77)


def _mask(m, c, state=STATE):
    from oracle import philox_ref
    mask = _ops().dropout_mask(1, m, c, state[0], state[1], state[2], DEV)[0]
    assert np.array_equal(mask.cpu().numpy(), philox_ref.dropout_mask(1, m, c, *state)[0])
    return mask


@pytest.mark.parametrize("m,n,k", SHAPES_H)
def test_site_h_image_is_the_image_of_the_masked_result(m, n, k):
    """snf_gemm_hl_ws_dropout_bf16, relu -> hl image: == split_hl(relu(A W^T + b) * mask tensor), bit for bit."""
    ops = _ops()
    a_hl, w_hl, bias, _ = _operands(m, n, k, m + n)
    plain = ops.gemm_hl(a_hl, w_hl, bias, "relu")
    got = ops.gemm_hl_dropout(a_hl, w_hl, bias, STATE, "relu", hl_out=True)
    assert torch.equal(got, ops.split_hl_rows(plain * _mask(m, n)))
    # p = 0 through the same entry point is the plain launch
    assert torch.equal(ops.gemm_hl_dropout(a_hl, w_hl, bias, (0.0, 1, 2), "relu", hl_out=True), ops.gemm_hl(a_hl, w_hl, bias, "relu", hl_out=True))


@pytest.mark.parametrize("m,n,k", SHAPES_Z)
def test_site_z_result_is_residual_plus_masked_result(m, n, k):
    """snf_gemm_hl_ws_dropout_bf16, fp32 output with a residual: == resid + (A W^T + b) * mask tensor, bit for bit -- the mask of an
    element does not depend on the tiling or on who runs the epilogue (the last shape runs split-K)."""
    ops = _ops()
    a_hl, w_hl, bias, g = _operands(m, n, k, m + n + 1)
    resid = torch.randn(m, n, generator=g).to(DEV)
    split = int(ops._ffi.load().snf_gemm_hl_ws_bytes(m, n, k)) > 0
    assert split == (m > 8000), "the split-K case must split, the others must not"
    plain = ops.gemm_hl(a_hl, w_hl, bias)
    mask = _mask(m, n)
    got = ops.gemm_hl_dropout(a_hl, w_hl, bias, STATE, resid=resid)
    assert torch.equal(got, resid + plain * mask)
    assert torch.equal(ops.gemm_hl_dropout(a_hl, w_hl, bias, STATE), plain * mask)
    assert torch.equal(ops.gemm_hl_dropout(a_hl, w_hl, bias, (0.0, 1, 2), resid=resid), ops.gemm_hl(a_hl, w_hl, bias, resid=resid))
    # the backward's pass over dz regenerates the same mask: image and column sums of mask * dz
    if n <= 8192:
        img, cs = ops.split_hl_colsum(resid, dropout=STATE)
        want_img, want_cs = ops.split_hl_colsum(resid * mask)
        assert torch.equal(img, want_img) and torch.equal(cs, want_cs)


def test_forms_that_do_not_exist_are_errors():
    ops = _ops()
    a_hl, w_hl, bias, _ = _operands(256, 256, 64, 3)
    with pytest.raises(ValueError):
        ops.gemm_hl_dropout(a_hl, w_hl, bias, STATE, "gelu", hl_out=True)
    out = torch.empty(256, 256, dtype=torch.float32, device=DEV)
    lib = ops._ffi.load()
    rc = lib.snf_gemm_hl_dropout_bf16(ops._p(a_hl), a_hl.stride(0), ops._p(w_hl), w_hl.stride(0), ops._p(bias), None, 0, 256, 256, 64,
                                      ops.ACT_CODES["gelu"], ops._p(out), 256, ops.DT_F32, 0.1, 1, 2, ops._stream())
    assert rc != 0          # a missing kernel is an error, never another kernel


def test_mask_statistics():
    """[4096, 3072] at p = 0.1, from the binomial: kept fraction within 5 sigma of 0.9; two offsets agree on a fraction within 5 sigma of
    0.9^2 + 0.1^2 = 0.82; one state gives one mask."""
    ops = _ops()
    cnt = 4096 * 3072
    assert cnt == 12582912
    a = ops.dropout_mask(1, 4096, 3072, 0.1, 99, 1000, DEV)
    b = ops.dropout_mask(1, 4096, 3072, 0.1, 99, 1001, DEV)
    kept = float((a > 0).double().mean())
    assert abs(kept - 0.9) <= 5 * math.sqrt(0.09 / cnt), kept
    agree = float(((a > 0) == (b > 0)).double().mean())
    assert abs(agree - 0.82) <= 5 * math.sqrt(0.82 * 0.18 / cnt), agree
    assert torch.equal(a, ops.dropout_mask(1, 4096, 3072, 0.1, 99, 1000, DEV))
    assert set(torch.unique(a).tolist()) == {0.0, float(np.float32(1.0 / (1.0 - np.float64(np.float32(0.1)))))}


@pytest.mark.parametrize("n,d,h,lam", [(16384, 768, 6, 200), (16391, 768, 6, 200)])
def test_fused_chain_with_encoder_dropout_matches_the_restated_layer(n, d, h, lam, monkeypatch):
    """Logits and every parameter gradient of EncoderLayer0X3Fn with encoder_dropout = 0.1 in train mode against the restated layer fed
    with the mask tensors of layer.last_dropout_states.  Comparators and bounds are those of
    test_fused_x3_layer0_training_matches_the_generic_fp32_chain in train mode: fp32 library GEMMs (5e-5 / 2e-4), x3 operands
    (5e-5 / 5e-4), and -- where that test has the concatenated-K chain, which declines encoder dropout -- the layer in float64 at that
    comparator's bounds (5e-5 / 2e-4); 3e-3 / 5e-3 for its gate_keys / small_keys."""
    from snuffy_amd import autograd as SA
    from snuffy_amd import functional as SF
    sd = _perturbed_state_dict(n, d, h, lam)
    x = torch.randn(1, n, d, device=DEV)
    assert SA._x3_train_hl_ok(n, d, 4 * d)

    def run(gemm, layer_fn=None):
        monkeypatch.setattr(SF, "FP32_GEMM", gemm)
        if layer_fn is not None:
            monkeypatch.setattr(SA, "encoder_layer_train", layer_fn)
        net = build_amd_milnet(d, h, "relu", lam, 0.0, 1, enc_drop=0.1)
        net.load_state_dict(sd, strict=True)
        net = net.to(DEV).configure(precision="fp32", return_attention=False)
        net.train(True)
        torch.manual_seed(11)
        np.random.seed(5)
        ins, logits, _ = net(x)
        (logits.sum() * 3 + ins.max()).backward()
        return net, {k: p.grad.float().clone() for k, p in net.named_parameters()}, logits.detach().clone()

    calls = []
    real_apply = SA.EncoderLayer0X3Fn.apply
    monkeypatch.setattr(SA.EncoderLayer0X3Fn, "apply", lambda *a: (calls.append(1), real_apply(*a))[1])
    net, g_fused, out_fused = run("x3")
    assert calls, "the fused chain declined a layer with encoder dropout"
    states = net.b_classifier.encoder.layers[0].last_dropout_states
    assert all(states[s] is not None and states[s][0] == 0.1 for s in ("attn", "A", "H", "Z"))
    assert len({states[s][2] for s in states}) == 4            # one Philox offset per site
    gate_keys = ("feed_forward.w_1.weight", "feed_forward.w_1.bias", "sublayer.1.norm.weight", "sublayer.1.norm.bias")
    small_keys = ("linears.0.weight", "linears.0.bias", "linears.1.weight", "sublayer.0.norm.weight")
    for other, gemm, bound_out, bound in (("library", "library", 5e-5, 2e-4), ("x3", "x3", 5e-5, 5e-4), ("fp64", "library", 5e-5, 2e-4)):
        _, g_ref, out_ref = run(gemm, _restated_layer(states, other))
        err_out = (out_fused - out_ref).abs().max().item() / max(1.0, out_ref.abs().max().item())
        print("encoder dropout parity n=%d vs %s: logits %.3e" % (n, other, err_out))
        rels = {}
        for k in g_fused:
            if k.endswith("self_attn.linears.1.bias"):
                continue                           # mathematically zero gradient
            a, b = g_fused[k].double(), g_ref[k].double()
            rels[k] = float((a - b).norm() / b.norm().clamp_min(1e-12))
            print("    %-55s %.3e" % (k, rels[k]))
        assert err_out <= bound_out, (other, err_out)
        for k, rel in rels.items():
            assert rel < (5e-3 if k.endswith(small_keys) else 3e-3 if k.endswith(gate_keys) else bound), (k, other, rel)


def test_without_encoder_dropout_the_switch_changes_nothing(monkeypatch):
    """encoder_dropout = 0 in train mode: logits and gradients are torch.equal with FUSED_X3_ENCODER_DROPOUT on and off."""
    from snuffy_amd import autograd as SA
    n, d, h, lam = 16384, 768, 6, 200
    sd = _perturbed_state_dict(n, d, h, lam)
    x = torch.randn(1, n, d, device=DEV)
    res = {}
    for switch in (True, False):
        monkeypatch.setattr(SA, "FUSED_X3_ENCODER_DROPOUT", switch)
        net = build_amd_milnet(d, h, "relu", lam, 0.0, 1, enc_drop=0.0)
        net.load_state_dict(sd, strict=True)
        net = net.to(DEV).configure(precision="fp32", return_attention=False)
        net.train(True)
        torch.manual_seed(11)
        np.random.seed(5)
        ins, logits, _ = net(x)
        (logits.sum() * 3 + ins.max()).backward()
        res[switch] = (logits.detach().clone(), {k: p.grad.clone() for k, p in net.named_parameters()})
        st = net.b_classifier.encoder.layers[0].last_dropout_states
        assert st["attn"] is not None and st["A"] is None and st["H"] is None and st["Z"] is None      # a site with p == 0 draws nothing
    assert torch.equal(res[True][0], res[False][0])
    for k in res[True][1]:
        assert torch.equal(res[True][1][k], res[False][1][k]), k


def test_trainer_step_with_encoder_dropout_reaches_the_fused_chain(monkeypatch):
    """One epoch of two synthetic bags through train.Snuffy (a SmallWeightTrainer) with --encoder_dropout 0.1: every step runs
    EncoderLayer0X3Fn, the loss and every gradient are finite."""
    from snuffy_amd import autograd as SA
    from snuffy_amd.train import Snuffy, get_args_parser
    torch.manual_seed(0)
    np.random.seed(0)
    a = get_args_parser().parse_args(["--encoder_dropout", "0.1"])
    a.feats_size, a.num_heads, a.big_lambda, a.optimizer, a.num_epochs = 768, 6, 200, "adamw", 1
    tr = Snuffy(a)
    layer = tr.milnet.b_classifier.encoder.layers[0]
    assert layer.sublayer[0].dropout.p == 0.1 and layer.sublayer[1].dropout.p == 0.1 and layer.feed_forward.dropout.p == 0.1
    calls, grads_ok = [], []
    real_apply = SA.EncoderLayer0X3Fn.apply
    monkeypatch.setattr(SA.EncoderLayer0X3Fn, "apply", lambda *args: (calls.append(1), real_apply(*args))[1])
    real_after = tr._after_run_model_in_training_mode

    def after(**kw):
        grads_ok.append(all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in tr.milnet.parameters()))
        return real_after(**kw)

    monkeypatch.setattr(tr, "_after_run_model_in_training_mode", after)
    g = np.random.RandomState(3)
    feats = [g.randn(16384, 768).astype(np.float32), g.randn(16391, 768).astype(np.float32)]
    feats[1][:50] += 1.0
    labels = [np.array([0.0], dtype=np.float32), np.array([1.0], dtype=np.float32)]
    res = tr.train((labels, feats, None, None), 1)
    assert len(calls) == 2 and grads_ok == [True, True]
    assert np.isfinite(res["epoch_train_loss"])
    assert all(bool(torch.isfinite(p).all()) for p in tr.milnet.parameters())
