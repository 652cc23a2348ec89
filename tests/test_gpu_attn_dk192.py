"""The bf16 MFMA sparse attention at head width 192 (the reference README's MAE recipe: D = 768, h = 4, Lambda = 500 as 250 top + 250
random): the forward kernels (one launch holds 128 keys, up to 8 key chunks), in-kernel dropout, the backward over key chunks
(the only backward built for dk = 192), bf16 inference of the model on the new route, and EncoderLayer0Bf16Fn at the recipe's layer.
Tolerances and helpers are those of tests/test_gpu_kernels.py::test_sparse_attn_mfma, tests/test_gpu_attn_key_chunks.py and
tests/test_gpu_encoder_dropout_bf16.py, unchanged."""
import math

import numpy as np
import pytest
import torch

from oracle import snuffy_oracle as orc
from tests.attn_widths import DROP_OFFSET, DROP_SEED, P_DROP, TRAIN_192 as ROW
from tests.helpers import (TOL, ReplayRNG, _c_backward, _ops, _parity, _perturbed_state_dict, _qv, _ref, _run, attn_ref, bf16r,
                           build_amd_milnet, rel_err, synth_state)
from tests.helpers import grad_close as _close

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
DK = ROW.dk

# (n, k, h): smallest possible; one partly filled tile, one key block; two row tiles, 4th key block partly filled; exactly one full
# chunk; two chunks, the second nearly empty (2 key blocks); the recipe's keys and heads; eight full chunks
SHAPES = ROW.SHAPES
# more row tiles than compute units: workgroups straddle heads
BIG = ROW.BIG


@pytest.mark.parametrize("n,k,h,dt", [s + (dt,) for s in SHAPES for dt in ("f32", "bf16")] + [BIG + ("bf16",)])
def test_forward(n, k, h, dt):
    """The checks of test_sparse_attn_mfma at dk = 192.  Before the dk = 192 kernels the first call raises the library's "unsupported
    shape" error."""
    ops = _ops()
    assert getattr(ops, ROW.supported)(k, n, 2 * h * DK)
    g = torch.Generator().manual_seed(n * 3 + k)
    d = h * DK
    q, kp, v = torch.randn(n, d, generator=g), torch.randn(k, d, generator=g), torch.randn(n, d, generator=g)
    tdt = torch.float32 if dt == "f32" else BF
    qd, vd = _qv(q, v, dt)                                                   # row-strided halves of one [n, 2d] buffer
    o, attn, lse = getattr(ops, ROW.single)(qd, vd, kp.to(DEV), n, h, need_attn=True, need_lse=True)
    # (a) against the exact oracle: bf16-class tolerance
    o_ref, p_ref = attn_ref(q, kp, v, h)
    assert (attn.cpu().double() - p_ref).abs().max() < 1e-2
    assert rel_err(o.cpu(), o_ref) < 1e-2
    # (b) against the oracle fed with the same bf16-rounded operands: tight (catches any layout slip)
    o_r, p_r = attn_ref(bf16r(q), bf16r(kp), bf16r(v), h)
    assert (attn.cpu().double() - p_r).abs().max() < 2e-5 + 2e-3 * float(p_r.max())
    assert rel_err(o.cpu(), o_r) < 3e-3
    # rows of P sum to one; sum over keys of O equals the column sums of V
    assert (attn.sum(-1) - 1).abs().max() < 1e-4
    assert rel_err(o.cpu().view(k, h, DK).sum(0), bf16r(v).view(n, h, DK).sum(0)) < 5e-3
    # lse against the oracle on the rounded operands
    s_r = (bf16r(q).double().view(n, h, DK).transpose(0, 1) @ bf16r(kp).double().view(k, h, DK).transpose(0, 1).transpose(1, 2)) / DK ** 0.5
    assert (lse.cpu().double() - torch.logsumexp(s_r, -1)).abs().max() < 1e-3
    # run-to-run determinism, contiguous operands
    o2, attn2, _ = getattr(ops, ROW.single)(q.to(DEV).to(tdt), v.to(DEV).to(tdt), kp.to(DEV), n, h, need_attn=True)
    assert torch.equal(o2, o) and torch.equal(attn2, attn)
    # without materialising A (need_attn=False, with and without lse) the output is the same
    o3, a3, l3 = getattr(ops, ROW.single)(qd, vd, kp.to(DEV), n, h)
    assert a3 is None and l3 is None and (torch.equal(o3, o) or rel_err(o3.cpu(), o.cpu()) < 2e-3)
    o5, a5, l5 = getattr(ops, ROW.single)(qd, vd, kp.to(DEV), n, h, need_attn=False, need_lse=True)
    assert a5 is None and torch.equal(l5, lse) and torch.equal(o5, o)
    # a bf16 Kp is read as it is: same bits as the library's own round-to-nearest-even of the f32 Kp
    o4, a4, _ = getattr(ops, ROW.single)(qd, vd, kp.to(DEV).to(BF), n, h, need_attn=True)
    assert torch.equal(o4, o) and torch.equal(a4, attn)


@pytest.mark.parametrize("n,k,h,dt", ROW.DROP_SHAPES)
def test_dropout_forward_and_backward(n, k, h, dt):
    """test_dropout_over_key_chunks_forward_and_backward at dk = 192: lse is the undropped forward's, A = P o M bit for bit with the host
    Philox mask, O within 3e-3 of fp64 with that mask; the backward with (p, seed, offset) equals the backward fed with the mask tensor,
    both within 1.5e-2 of fp64 autograd.  The forward's chunks (128 keys) and the backward's (192) differ; the mask is keyed on the
    key index among all keys."""
    from oracle import philox_ref
    ops = _ops()
    p_drop, seed, offset = P_DROP, DROP_SEED, DROP_OFFSET
    g = torch.Generator().manual_seed(n + k)
    d = h * DK
    q, kp, v, dout = (torch.randn(s, d, generator=g) for s in (n, k, n, k))
    qd_, vd_ = _qv(q, v, dt)
    mask = torch.from_numpy(philox_ref.dropout_mask(h, n, k, p_drop, seed, offset))
    o, attn, lse = getattr(ops, ROW.single)(qd_, vd_, kp.to(DEV), n, h, need_attn=True, need_lse=True, dropout=(p_drop, seed, offset))
    o0, attn0, lse0 = getattr(ops, ROW.single)(qd_, vd_, kp.to(DEV), n, h, need_attn=True, need_lse=True)
    assert torch.equal(lse, lse0)
    assert torch.equal(attn.cpu(), attn0.cpu() * mask)
    qr, kr, vr = bf16r(q), bf16r(kp), bf16r(v)
    qh, kh, vh = (t.double().view(-1, h, DK).transpose(0, 1) for t in (qr, kr, vr))
    p_r = torch.softmax(qh @ kh.transpose(1, 2) / DK ** 0.5, dim=-1)
    o_r = ((p_r * mask.double()).transpose(1, 2) @ vh).transpose(0, 1).reshape(k, d)
    err_o = rel_err(o.cpu(), o_r)
    o1, _, _ = getattr(ops, ROW.single)(qd_, vd_, kp.to(DEV), n, h, need_attn=False, need_lse=True, dropout=(p_drop, seed, offset))
    assert torch.equal(o1, o)
    dq, dkp, dv = ops.sparse_attn_bwd_mfma(qd_, vd_, kp.to(DEV), dout.to(DEV), lse, h, dropout=(p_drop, seed, offset))
    dq2, dkp2, dv2 = ops.sparse_attn_bwd_mfma(qd_, vd_, kp.to(DEV), dout.to(DEV), lse, h, mask=mask.to(DEV))
    rq, rk, rv, _ = _ref(qr, kr, vr, bf16r(dout), h, mask)
    errs = [rel_err(got.cpu(), want) for got, want in ((dq, rq), (dkp, rk), (dv, rv))]
    print("dk192 dropout %s %s: O %.3e  dq %.3e dkp %.3e dv %.3e" % ((n, k, h), dt, err_o, *errs))
    assert err_o < 3e-3
    assert torch.equal(dq, dq2) and torch.equal(dkp, dkp2) and torch.equal(dv, dv2)
    assert max(errs) < 1.5e-2, errs


@pytest.mark.parametrize("drop", [0.0, 0.25])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("n,k,h", SHAPES)
def test_backward(n, k, h, dt, drop):
    """test_backward_over_key_chunks_against_fp64_autograd at dk = 192 (one chunk included: dk = 192 has no single-launch backward):
    1.5e-2 against fp64 autograd on the bf16-rounded operands, 2e-2 on the exact ones; repeat calls are bit-identical; the bf16 outputs are
    the fp32 ones rounded once; with f32 operands every dS column is written and |sum_j dS| <= 2^-7 sum_j |P_j dP_j| * scale (derived
    there)."""
    ops = _ops()
    g = torch.Generator().manual_seed(7 * n + k)
    d = h * DK
    q, kp, v = (torch.randn(s, d, generator=g) for s in (n, k, n))
    dout = torch.randn(k, d, generator=g)
    mask = (torch.rand(h, n, k, generator=g) >= drop).float() / (1.0 - drop) if drop > 0 else None
    mask_d = None if mask is None else mask.to(DEV)
    qd_, vd_ = _qv(q, v, dt)
    _, _, lse = getattr(ops, ROW.single)(qd_, vd_, kp.to(DEV), n, h, need_lse=True)
    dq, dkp, dv = ops.sparse_attn_bwd_mfma(qd_, vd_, kp.to(DEV), dout.to(DEV), lse, h, mask=mask_d)
    print("dk192 backward %s %s drop %.2f" % ((n, k, h), dt, drop))
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
        assert bool(torch.isfinite(ds).all())                            # every column of every chunk was written (NaN pre-fill)
        rowsum = ds.double().sum(-1).abs().cpu()
        bound = 2.0 ** -7 * pdp / math.sqrt(DK)
        worst = float((rowsum / bound.clamp_min(1e-30)).max())
        print("    sum_j dS: max %.3e, worst ratio to the bound %.3f" % (float(rowsum.max()), worst))
        assert bool((rowsum <= bound + 1e-9).all()), worst


def test_single_launch_backward_keeps_refusing_dk192():
    ops = _ops()
    n, k, h = 64, 32, 1
    g = torch.Generator().manual_seed(0)
    q, kp, v, dout = (torch.randn(s, h * DK, generator=g) for s in (n, k, n, k))
    qd_, vd_ = _qv(q, v, "bf16")
    _, _, lse = getattr(ops, ROW.single)(qd_, vd_, kp.to(DEV), n, h, need_lse=True)
    with pytest.raises(Exception, match="unsupported shape"):
        _c_backward("ex", qd_, vd_, kp.to(DEV), dout.to(DEV), lse, h)


def test_model_inference_on_the_dk192_route(monkeypatch):
    """bf16 inference of the MAE-recipe model (D = 768, h = 4, Lambda = 500 as 250 top + 250 random, N = 3000) in the pattern of
    test_readme_recipes_vs_oracle: the selection bit-exact, logits and sampled rows of A within TOL["bf16"] of the oracle on the MFMA
    route.  With MFMA_ATTN_DK192 off the forward is the previous routing's (fp32 copies of Q | V into the exact kernel: no MFMA
    attention launch), bit-identical run to run, inside the same bound, and the new route is within TOL["bf16"] of it."""
    from snuffy_amd import functional as SF
    from snuffy_amd import ops
    N, D, h, lam, r = 3000, ROW.D, ROW.H, ROW.LAM, 0.5
    net = synth_state(D, h, 1)
    layer = net.b_classifier.encoder.layers[0]
    layer.big_lambda, layer.random_patch_share, layer.top_big_lambda_share = lam, r, 1.0 - r
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    x = torch.randn(N, D, generator=torch.Generator().manual_seed(77))
    x = x / x.norm(dim=1, keepdim=True)
    _, logits_ref, p_ref, sels = orc.milnet_forward(x, sd, h, "relu", lam, r, 1, ReplayRNG(9))
    net = net.to(DEV).eval().configure(precision="bf16", return_attention=True)
    calls, exact = [], []
    real, real_exact = ops.sparse_attn_fwd_mfma, ops.sparse_attn_fwd
    monkeypatch.setattr(ops, "sparse_attn_fwd_mfma", lambda *a, **kw: (calls.append(tuple(a[2].shape)), real(*a, **kw))[1])
    monkeypatch.setattr(ops, "sparse_attn_fwd", lambda *a, **kw: (exact.append(a[0].dtype), real_exact(*a, **kw))[1])
    tol = TOL["bf16"]
    rows = torch.arange(0, N, 53)

    def run():
        np.random.seed(9)
        with torch.no_grad():
            _, logits, A = net(x.to(DEV).unsqueeze(0))
        top, rnd = layer.last_selection
        assert np.array_equal(torch.cat((top, rnd)).cpu().numpy(), sels[0].numpy()) and top.numel() == 250 and rnd.numel() == 250
        assert (logits.cpu()[0] - logits_ref).abs().max() < tol
        assert (A[0][:, rows.to(DEV), :].cpu() - p_ref[:, rows, :]).abs().max() < tol
        assert (A.sum(-1) - 1).abs().max() < 1e-4
        return logits, A

    monkeypatch.setattr(SF, ROW.single_switch, True)
    logits, A = run()
    assert calls == [(lam, D)] and not exact                              # the MFMA attention, no fp32 copies into the exact kernel
    del calls[:]
    monkeypatch.setattr(SF, ROW.single_switch, False)
    logits0, A0 = run()
    logits1, A1 = run()
    assert not calls and exact == [torch.float32, torch.float32]          # the previous routing
    assert torch.equal(logits0, logits1) and torch.equal(A0, A1)
    print("dk192 inference: new route vs previous routing: logits %.3e, A %.3e" % ((logits - logits0).abs().max().item(),
                                                                                  (A - A0).abs().max().item()))
    assert (logits - logits0).abs().max().item() < tol and (A - A0).abs().max().item() < tol


@pytest.mark.parametrize("sites", [(0.0, 0.0, 0.0), (0.1, 0.1, 0.1)])
def test_chain_at_dk192_matches_the_restated_layer(sites, monkeypatch):
    """One training step through EncoderLayer0Bf16Fn (asserted by the spy inside _parity) on the D = 768 / h = 4 / Lambda = 500 layer at
    N = 3000 against the plain-torch restatement, with the bounds and the widening rule of tests/test_gpu_encoder_dropout_bf16.py; then,
    with FUSED_BF16_DK192 off, the same step takes the generic chain."""
    from snuffy_amd import autograd as SA
    n, d, h, lam = 3000, ROW.D, ROW.H, ROW.LAM
    assert d // h == DK
    monkeypatch.setattr(SA, ROW.train_switch, True)
    _parity(monkeypatch, n, d, h, lam, sites=sites)
    calls = []
    real_apply = SA.EncoderLayer0Bf16Fn.apply
    monkeypatch.setattr(SA.EncoderLayer0Bf16Fn, "apply", lambda *a: (calls.append(1), real_apply(*a))[1])
    sd = _perturbed_state_dict(n, d, h, lam)
    x = torch.randn(1, n, d, device=DEV)
    net, grads, logits = _run(monkeypatch, sd, x, d, h, lam, "bf16", 0.0, sites=sites)
    assert calls and bool(torch.isfinite(logits).all())
    params = dict(net.named_parameters())
    for k_, g_ in grads.items():                                          # parameter gradient shapes are unchanged
        assert g_.shape == params[k_].shape and bool(torch.isfinite(g_).all()), k_
    del calls[:]
    monkeypatch.setattr(SA, ROW.train_switch, False)
    _, grads0, logits0 = _run(monkeypatch, sd, x, d, h, lam, "bf16", 0.0, sites=sites)
    assert not calls and bool(torch.isfinite(logits0).all())
    assert sorted(grads0) == sorted(grads)


def test_stepper_step_takes_the_chain_at_dk192_and_the_switch_takes_it_out(monkeypatch):
    """One optimizer step of the training driver (BagParallelStepper, bf16) on the MAE-recipe model: the fused chain runs, the loss is
    finite, the state_dict keeps its keys and shapes; with FUSED_BF16_DK192 off the same step takes the generic chain."""
    from snuffy_amd import autograd as SA
    from snuffy_amd.train import BagParallelStepper
    n, d, h, lam = 3000, ROW.D, ROW.H, ROW.LAM
    sd = _perturbed_state_dict(n, d, h, lam)
    calls = []
    real_apply = SA.EncoderLayer0Bf16Fn.apply
    monkeypatch.setattr(SA.EncoderLayer0Bf16Fn, "apply", lambda *a: (calls.append(1), real_apply(*a))[1])
    for on in (True, False):
        monkeypatch.setattr(SA, ROW.train_switch, on)
        net = build_amd_milnet(d, h, "relu", lam, 0.5, 1, enc_drop=0.1)
        net.load_state_dict(sd, strict=True)
        net = net.to(DEV)
        st = BagParallelStepper(net, world_size=1, dist=None, device=torch.device(DEV, 0), precision="bf16")
        torch.manual_seed(1)
        np.random.seed(1)
        x = torch.randn(1, n, d, device=DEV)
        del calls[:]
        out = st.step(x, torch.tensor([1.0], device=DEV))
        torch.cuda.synchronize()
        assert bool(calls) is on
        loss = out[0] if isinstance(out, (tuple, list)) else out
        if isinstance(loss, torch.Tensor):
            assert bool(torch.isfinite(loss).all())
        assert list(net.state_dict().keys()) == list(sd.keys())
        for k_, t in net.state_dict().items():
            assert t.shape == sd[k_].shape and bool(torch.isfinite(t).all()), k_
