"""The fused bf16 training chain above one key chunk of the MFMA attention and at padded head widths: the backward over key chunks
(snf_sparse_attn_bwd_mfma_chunked) against fp64 autograd, in-kernel dropout in the forward over key chunks, and EncoderLayer0Bf16Fn at
Lambda = 300 / 500 (two and three chunks; dk = 96 padded to 128) against the plain-torch restatement of the layer."""
import math

import pytest
import torch

from tests.helpers import BF, DEV, _c_backward, _ops, _parity, _perturbed_state_dict, _qv, _ref, _run, bf16r, rel_err
from tests.helpers import grad_close as _close

pytestmark = pytest.mark.gpu


# a last chunk of few keys, exactly full chunks, the README's 500 and 900 keys, K % 4 != 0 (scalar dS stores, fp32 dS)
SHAPES = [(129, 225, 2, 128), (300, 448, 2, 128), (1000, 500, 4, 128), (640, 900, 2, 128), (257, 451, 1, 128),
          (300, 257, 3, 64), (1000, 500, 6, 64)]


@pytest.mark.parametrize("drop", [0.0, 0.25])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("n,k,h,dk", SHAPES)
def test_backward_over_key_chunks_against_fp64_autograd(n, k, h, dk, dt, drop):
    """ops.sparse_attn_bwd_mfma above one key chunk, as test_sparse_attn_bwd_mfma checks it below: 1.5e-2 against fp64 autograd on the
    bf16-rounded operands, 2e-2 on the exact ones; repeat calls are bit-identical; the bf16 outputs are the fp32 ones rounded once.

    f32 operands also: sum_j dS[a, i, j] = 0 in exact arithmetic (D is the row sum over ALL keys; a D taken per chunk leaves
    -P(chunk) * D(other chunks), of the order of the terms themselves).  The kernels build dS from the fp32 P and dP with
    D = sum_j bf16(P_j M_j) dP_j (P o M is the bf16 MFMA operand of dV, relative rounding 2^-9), so the sum is at most
    2^-9 sum_j |P_j dP_j| * scale plus fp32 rounding of lse and exp2 (1e-5 of the same): the bound is 2^-7 sum_j |P_j dP_j| * scale."""
    ops = _ops()
    assert not ops.mfma_attn_bwd_supported(k, dk) and ops.mfma_attn_train_chunks_supported(k, dk)
    g = torch.Generator().manual_seed(7 * n + k)
    d = h * dk
    q, kp, v = (torch.randn(s, d, generator=g) for s in (n, k, n))
    dout = torch.randn(k, d, generator=g)
    mask = (torch.rand(h, n, k, generator=g) >= drop).float() / (1.0 - drop) if drop > 0 else None
    mask_d = None if mask is None else mask.to(DEV)
    qd_, vd_ = _qv(q, v, dt)
    _, _, lse = ops.sparse_attn_fwd_mfma(qd_, vd_, kp.to(DEV), n, h, need_lse=True)
    dq, dkp, dv = ops.sparse_attn_bwd_mfma(qd_, vd_, kp.to(DEV), dout.to(DEV), lse, h, mask=mask_d)
    print("backward over key chunks %s %s drop %.2f" % ((n, k, h, dk), dt, drop))
    rq, rk, rv, pdp = _ref(bf16r(q), bf16r(kp), bf16r(v), bf16r(dout), h, mask)
    for got, want, name in ((dq, rq, "dq"), (dkp, rk, "dkp"), (dv, rv, "dv")):
        _close(got, want, 1.5e-2, name)
    eq, ek, ev, _ = _ref(q, kp, v, dout, h, mask)
    for got, want, name in ((dq, eq, "dq"), (dkp, ek, "dkp"), (dv, ev, "dv")):
        _close(got, want, 2e-2, name)
    dq2, dkp2, dv2 = ops.sparse_attn_bwd_mfma(qd_, vd_, kp.to(DEV), dout.to(DEV), lse, h, mask=mask_d)
    assert torch.equal(dq, dq2) and torch.equal(dkp, dkp2) and torch.equal(dv, dv2)
    dq3, dkp3, dv3 = ops.sparse_attn_bwd_mfma(qd_, vd_, kp.to(DEV), dout.to(DEV), lse, h, mask=mask_d, fused_bf16_grads=True)
    assert dq3._base is dv3._base and dq3._base.shape == (n, 2 * d) and dq3.dtype == BF
    assert torch.equal(dq3, dq.to(BF)) and torch.equal(dv3, dv.to(BF)) and torch.equal(dkp3, dkp)
    if dt == "f32":
        cq, cv, ds = _c_backward("chunked", qd_, vd_, kp.to(DEV), dout.to(DEV), lse, h, mask=mask_d)
        assert torch.equal(cq, dq) and torch.equal(cv, dv)
        assert bool(torch.isfinite(ds).all())                            # every column of every chunk was written
        rowsum = ds.double().sum(-1).abs().cpu()
        bound = 2.0 ** -7 * pdp / math.sqrt(dk)
        worst = float((rowsum / bound.clamp_min(1e-30)).max())
        print("    sum_j dS: max %.3e, worst ratio to the bound %.3f" % (float(rowsum.max()), worst))
        assert bool((rowsum <= bound + 1e-9).all()), worst


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("n,k,h,dk", [(3000, 224, 2, 128), (2048, 256, 6, 64)])
def test_one_chunk_is_the_single_launch_kernel_bit_for_bit(n, k, h, dk, dt):
    ops = _ops()
    g = torch.Generator().manual_seed(n + k)
    d = h * dk
    q, kp, v, dout = (torch.randn(s, d, generator=g) for s in (n, k, n, k))
    qd_, vd_ = _qv(q, v, dt)
    _, _, lse = ops.sparse_attn_fwd_mfma(qd_, vd_, kp.to(DEV), n, h, need_lse=True)
    for drop in ((0.0, 0, 0), (0.1, 99, 3)):
        a = _c_backward("chunked", qd_, vd_, kp.to(DEV), dout.to(DEV), lse, h, drop=drop)
        b = _c_backward("ex", qd_, vd_, kp.to(DEV), dout.to(DEV), lse, h, drop=drop)
        for x, y, name in zip(a, b, ("dq", "dv", "ds")):
            assert torch.equal(x, y), (name, drop)


@pytest.mark.parametrize("n,k,h,dk,dt", [(777, 300, 2, 128, "f32"), (1000, 500, 4, 128, "bf16"), (512, 260, 3, 64, "bf16")])
def test_dropout_over_key_chunks_forward_and_backward(n, k, h, dk, dt):
    """test_mfma_attention_dropout_forward_and_backward above one key chunk: lse is the undropped forward's, A = P o M bit for bit with
    the host Philox mask, O within 3e-3 of fp64 with that mask; the backward with (p, seed, offset) equals the backward fed with the mask
    tensor, both within 1.5e-2 of fp64 autograd."""
    from oracle import philox_ref
    ops = _ops()
    p_drop, seed, offset = 0.1, 987654321, 5
    g = torch.Generator().manual_seed(n + k)
    d = h * dk
    q, kp, v, dout = (torch.randn(s, d, generator=g) for s in (n, k, n, k))
    qd_, vd_ = _qv(q, v, dt)
    mask = torch.from_numpy(philox_ref.dropout_mask(h, n, k, p_drop, seed, offset))
    o, attn, lse = ops.sparse_attn_fwd_mfma(qd_, vd_, kp.to(DEV), n, h, need_attn=True, need_lse=True, dropout=(p_drop, seed, offset))
    o0, attn0, lse0 = ops.sparse_attn_fwd_mfma(qd_, vd_, kp.to(DEV), n, h, need_attn=True, need_lse=True)
    assert torch.equal(lse, lse0)
    assert torch.equal(attn.cpu(), attn0.cpu() * mask)
    qr, kr, vr = bf16r(q), bf16r(kp), bf16r(v)
    qh, kh, vh = (t.double().view(-1, h, dk).transpose(0, 1) for t in (qr, kr, vr))
    p_r = torch.softmax(qh @ kh.transpose(1, 2) / dk ** 0.5, dim=-1)
    o_r = ((p_r * mask.double()).transpose(1, 2) @ vh).transpose(0, 1).reshape(k, d)
    err_o = rel_err(o.cpu(), o_r)
    # without attn / lse outputs behind the first chunk the later chunks still drop their probabilities
    o1, _, _ = ops.sparse_attn_fwd_mfma(qd_, vd_, kp.to(DEV), n, h, need_attn=False, need_lse=True, dropout=(p_drop, seed, offset))
    assert torch.equal(o1, o)
    dq, dkp, dv = ops.sparse_attn_bwd_mfma(qd_, vd_, kp.to(DEV), dout.to(DEV), lse, h, dropout=(p_drop, seed, offset))
    dq2, dkp2, dv2 = ops.sparse_attn_bwd_mfma(qd_, vd_, kp.to(DEV), dout.to(DEV), lse, h, mask=mask.to(DEV))
    rq, rk, rv, _ = _ref(qr, kr, vr, bf16r(dout), h, mask)
    errs = [rel_err(got.cpu(), want) for got, want in ((dq, rq), (dkp, rk), (dv, rv))]
    print("dropout over key chunks %s %s: O %.3e  dq %.3e dkp %.3e dv %.3e" % ((n, k, h, dk), dt, err_o, *errs))
    assert err_o < 3e-3
    assert torch.equal(dq, dq2) and torch.equal(dkp, dkp2) and torch.equal(dv, dv2)
    assert max(errs) < 1.5e-2, errs


# n, D, h, Lambda: dk 128, two chunks; dk 96 padded to 128, three chunks, a row tail; dk 64, two chunks
CHAIN = [(700, 256, 2, 300), (2051, 384, 4, 500), (1024, 384, 6, 300)]


@pytest.mark.parametrize("sites", [(0.0, 0.0, 0.0), (0.1, 0.1, 0.1)])
@pytest.mark.parametrize("n,d,h,lam", CHAIN)
def test_chain_above_one_key_chunk_matches_the_restated_layer(n, d, h, lam, sites, monkeypatch):
    """One training step through EncoderLayer0Bf16Fn (asserted by the spy inside _parity) against the plain-torch restatement fed with the
    mask tensors of layer.last_dropout_states, in fp32 and under bf16 autocast, with the bounds and the widening rule of
    tests/test_gpu_encoder_dropout_bf16.py."""
    from snuffy_amd import autograd as SA
    from snuffy_amd import functional as SF
    layer_dk = d // h
    assert SF.head_pad(layer_dk) in (64, 128) and lam > (224 if SF.head_pad(layer_dk) == 128 else 256)
    _parity(monkeypatch, n, d, h, lam, sites=sites)
    # the switch off: the generic autograd chain, as before
    calls = []
    real_apply = SA.EncoderLayer0Bf16Fn.apply
    monkeypatch.setattr(SA.EncoderLayer0Bf16Fn, "apply", lambda *a: (calls.append(1), real_apply(*a))[1])
    monkeypatch.setattr(SA, "FUSED_BF16_KEY_CHUNKS", False)
    sd = _perturbed_state_dict(n, d, h, lam)
    x = torch.randn(1, n, d, device=DEV)
    _, grads, logits = _run(monkeypatch, sd, x, d, h, lam, "bf16", 0.0, sites=sites)
    assert not calls and bool(torch.isfinite(logits).all())


def test_padded_chain_keeps_parameter_shapes_and_state_dict_keys(monkeypatch):
    """dk = 96 rides padded to 128 inside the chain only: every gradient has its parameter's own shape, and a bf16 step from a
    reference-keyed state_dict leaves the keys as they were."""
    from snuffy_amd import autograd as SA
    n, d, h, lam = 2051, 384, 4, 500
    sd = _perturbed_state_dict(n, d, h, lam)
    x = torch.randn(1, n, d, device=DEV)
    calls = []
    real_apply = SA.EncoderLayer0Bf16Fn.apply
    monkeypatch.setattr(SA.EncoderLayer0Bf16Fn, "apply", lambda *a: (calls.append(1), real_apply(*a))[1])
    net, grads, logits = _run(monkeypatch, sd, x, d, h, lam, "bf16", 0.1)
    assert calls
    params = dict(net.named_parameters())
    for k_, g_ in grads.items():
        assert g_.shape == params[k_].shape, k_
        assert bool(torch.isfinite(g_).all()), k_
    opt = torch.optim.SGD(net.parameters(), lr=1e-3)
    opt.step()
    assert list(net.state_dict().keys()) == list(sd.keys())
    for k_, t in net.state_dict().items():
        assert t.shape == sd[k_].shape, k_
