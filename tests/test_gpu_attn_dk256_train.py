"""bf16 training at head width 256 (the reference README's SimCLR ResNet-18 recipe: D = 512, h = 2, Lambda = 900 as 200 + 700): the
dropout form of the dk = 256 forward, the backward over key chunks at DK = 256 (the only backward built for the width), SparseAttnFn on
the MFMA kernels at the native widths (SPARSE_ATTN_FN_WIDE), and EncoderLayer0Bf16Fn at the recipe's layer (FUSED_BF16_DK256).
Tolerances and helpers are those of tests/test_gpu_attn_key_chunks.py, tests/test_gpu_attn_dk192.py and
tests/test_gpu_encoder_dropout_bf16.py, unchanged."""
import math

import numpy as np
import pytest
import torch

from tests.attn_widths import DROP_OFFSET, DROP_SEED, P_DROP, TRAIN_256 as ROW
from tests.helpers import _c_backward, _ops, _parity, _perturbed_state_dict, _qv, _ref, bf16r, build_amd_milnet, rel_err
from tests.helpers import grad_close as _close

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
DK = ROW.dk

# (n, k, h): smallest possible; one key block with a tail; two blocks, row-tile tail; four blocks, k % 4 != 0 (the scalar dS path);
# exactly one chunk; two chunks (forward 65 + 64: the second starts at key 65, off a multiple of 4; backward 96 + 33); the recipe's
# keys (forward 7 chunks of 113 and one of 109, starts at every residue mod 4; backward 7 x 128 + 4); eight full chunks
SHAPES = ROW.SHAPES
# more row tiles than compute units: workgroups straddle heads (bf16 only)
BIG = ROW.BIG
DROP_SHAPES = ROW.DROP_SHAPES
SEED, OFFSET = DROP_SEED, DROP_OFFSET


def _lse(q, v, kp, h):
    """The forward's lse: the dk = 256 forward takes bf16 Q and V only, and those are the values the backward's MFMAs see either way."""
    qb, vb = _qv(q, v, "bf16")
    return getattr(_ops(), ROW.single)(qb, vb, kp.to(DEV), h, need_lse=True)[2]


_CASES = {}


def _case(n, k, h, drop):
    """Operands, mask tensor and the fp64 references of one (shape, drop), computed once and shared by the operand types."""
    key = (n, k, h, drop)
    if key not in _CASES:
        g = torch.Generator().manual_seed(7 * n + k)
        d = h * DK
        q, kp, v = (torch.randn(s, d, generator=g) for s in (n, k, n))
        dout = torch.randn(k, d, generator=g)
        mask = (torch.rand(h, n, k, generator=g) >= drop).float() / (1.0 - drop) if drop > 0 else None
        rounded = _ref(bf16r(q), bf16r(kp), bf16r(v), bf16r(dout), h, mask)
        exact = _ref(q, kp, v, dout, h, mask)
        if (n, k, h) == BIG:                                                     # one operand type only: nothing to share, 1 GB to keep
            return q, kp, v, dout, mask, rounded, exact[:3]
        _CASES[key] = (q, kp, v, dout, mask, rounded, exact[:3])
    return _CASES[key]


_DROP_CASES = {}


def _drop_case(n, k, h):
    if (n, k, h) not in _DROP_CASES:
        from oracle import philox_ref
        g = torch.Generator().manual_seed(n + k)
        d = h * DK
        q, kp, v, dout = (torch.randn(s, d, generator=g) for s in (n, k, n, k))
        mask = torch.from_numpy(philox_ref.dropout_mask(h, n, k, P_DROP, SEED, OFFSET))
        _DROP_CASES[(n, k, h)] = (q, kp, v, dout, mask)
    return _DROP_CASES[(n, k, h)]


@pytest.mark.parametrize("n,k,h", DROP_SHAPES)
def test_dropout_forward(n, k, h):
    """lse is the undropped launch's bit for bit, A = P o M bit for bit with the host Philox mask, O within 3e-3 of fp64 on the
    bf16-rounded operands with that mask; need_attn off gives the same O; p = 0 through the new entry is the old entry.  Before the
    dropout form existed the first call raises (no dropout argument, no entry point)."""
    ops = _ops()
    q, kp, v, _, mask = _drop_case(n, k, h)
    d = h * DK
    qd_, vd_ = _qv(q, v, "bf16")
    kd = kp.to(DEV)
    o, attn, lse = getattr(ops, ROW.single)(qd_, vd_, kd, h, need_attn=True, need_lse=True, dropout=(P_DROP, SEED, OFFSET))
    o0, attn0, lse0 = getattr(ops, ROW.single)(qd_, vd_, kd, h, need_attn=True, need_lse=True)
    assert torch.equal(lse, lse0)
    assert torch.equal(attn.cpu(), attn0.cpu() * mask)
    qh, kh, vh = (bf16r(t).double().view(-1, h, DK).transpose(0, 1) for t in (q, kp, v))
    p_r = torch.softmax(qh @ kh.transpose(1, 2) / DK ** 0.5, dim=-1)
    o_r = ((p_r * mask.double()).transpose(1, 2) @ vh).transpose(0, 1).reshape(k, d)
    err_o = rel_err(o.cpu(), o_r)
    print("dk256 dropout forward %s: O %.3e" % ((n, k, h), err_o))
    assert err_o < 3e-3
    o1, a1, l1 = getattr(ops, ROW.single)(qd_, vd_, kd, h, need_attn=False, need_lse=True, dropout=(P_DROP, SEED, OFFSET))
    assert a1 is None and torch.equal(o1, o) and torch.equal(l1, lse)
    o2, attn2, lse2 = getattr(ops, ROW.single)(qd_, vd_, kd, h, need_attn=True, need_lse=True, dropout=(0.0, SEED, OFFSET))
    assert torch.equal(o2, o0) and torch.equal(attn2, attn0) and torch.equal(lse2, lse0)
    # dropout without lse or attn is refused, as at the family's entry; so is p outside [0, 1)
    with pytest.raises(Exception, match="dropout needs the lse"):
        getattr(ops, ROW.single)(qd_, vd_, kd, h, dropout=(P_DROP, SEED, OFFSET))
    with pytest.raises(Exception, match="outside"):
        getattr(ops, ROW.single)(qd_, vd_, kd, h, need_lse=True, dropout=(1.0, SEED, OFFSET))


@pytest.mark.parametrize("n,k,h", DROP_SHAPES)
def test_dropout_backward(n, k, h):
    """The backward fed (p, seed, offset) equals the backward fed the mask tensor bit for bit; both within 1.5e-2 of fp64 autograd.  The
    forward's chunks (113 keys at k = 900) and the backward's (multiples of 32) differ; the mask is keyed on the key index among all
    keys."""
    ops = _ops()
    q, kp, v, dout, mask = _drop_case(n, k, h)
    qd_, vd_ = _qv(q, v, "bf16")
    lse = _lse(q, v, kp, h)
    dq, dkp, dv = ops.sparse_attn_bwd_mfma(qd_, vd_, kp.to(DEV), dout.to(DEV), lse, h, dropout=(P_DROP, SEED, OFFSET))
    dq2, dkp2, dv2 = ops.sparse_attn_bwd_mfma(qd_, vd_, kp.to(DEV), dout.to(DEV), lse, h, mask=mask.to(DEV))
    rq, rk, rv, _ = _ref(bf16r(q), bf16r(kp), bf16r(v), bf16r(dout), h, mask)
    errs = [rel_err(got.cpu(), want) for got, want in ((dq, rq), (dkp, rk), (dv, rv))]
    print("dk256 dropout backward %s: dq %.3e dkp %.3e dv %.3e" % ((n, k, h), *errs))
    assert torch.equal(dq, dq2) and torch.equal(dkp, dkp2) and torch.equal(dv, dv2)
    assert max(errs) < 1.5e-2, errs


@pytest.mark.parametrize("drop", [0.0, 0.25])
@pytest.mark.parametrize("n,k,h,dt", [s + (dt,) for s in SHAPES for dt in ("f32", "bf16")] + [BIG + ("bf16",)])
def test_backward(n, k, h, dt, drop):
    """test_backward_over_key_chunks_against_fp64_autograd at dk = 256 (one chunk included: the width has no single-launch backward):
    1.5e-2 against fp64 autograd on the bf16-rounded operands, 2e-2 on the exact ones; repeat calls are bit-identical; the bf16 outputs are
    the fp32 ones rounded once; with f32 operands every dS column is written and |sum_j dS| <= 2^-7 sum_j |P_j dP_j| * scale (derived
    there).  Before DK = 256 was built the chunked entry raises "unsupported shape"."""
    ops = _ops()
    assert getattr(ops, ROW.supported)(k, n, 2 * h * DK)
    q, kp, v, dout, mask, (rq, rk, rv, pdp), (eq, ek, ev) = _case(n, k, h, drop)
    d = h * DK
    mask_d = None if mask is None else mask.to(DEV)
    qd_, vd_ = _qv(q, v, dt)
    lse = _lse(q, v, kp, h)
    dq, dkp, dv = ops.sparse_attn_bwd_mfma(qd_, vd_, kp.to(DEV), dout.to(DEV), lse, h, mask=mask_d)
    print("dk256 backward %s %s drop %.2f" % ((n, k, h), dt, drop))
    for got, want, name in ((dq, rq, "dq"), (dkp, rk, "dkp"), (dv, rv, "dv")):
        _close(got, want, 1.5e-2, name)
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


def test_single_launch_backward_keeps_refusing_dk256():
    n, k, h = 64, 32, 1
    g = torch.Generator().manual_seed(0)
    q, kp, v, dout = (torch.randn(s, h * DK, generator=g) for s in (n, k, n, k))
    qd_, vd_ = _qv(q, v, "bf16")
    lse = _lse(q, v, kp, h)
    with pytest.raises(Exception, match="unsupported shape"):
        _c_backward("ex", qd_, vd_, kp.to(DEV), dout.to(DEV), lse, h)


def _spies(monkeypatch):
    """Call records of the attention entry points SparseAttnFn chooses between."""
    ops = _ops()
    rec = {}
    for name in ("sparse_attn_fwd_mfma", "sparse_attn_fwd_mfma_dk256", "sparse_attn_bwd_mfma", "sparse_attn_fwd", "sparse_attn_fwd_x3",
                 "sparse_attn_bwd", "dropout_mask"):
        real = getattr(ops, name)
        rec[name] = []
        monkeypatch.setattr(ops, name, (lambda real, log: lambda *a, **kw: (log.append((a, kw)), real(*a, **kw))[1])(real, rec[name]))
    return rec


@pytest.mark.parametrize("dk,n,k,h", [(256, 300, 129, 2), (256, 640, 900, 2), (192, 300, 129, 2), (192, 640, 500, 4)])
def test_sparse_attn_fn_on_the_mfma_kernels(dk, n, k, h, monkeypatch):
    """SPARSE_ATTN_FN_WIDE on, bf16 operands: the MFMA forward with in-kernel dropout and the chunked backward run, no [h, N, K] mask
    tensor is made, nothing but (q16, kp, v16, lse) is saved, and dq, dkp, dv are within the kernel bound (1.5e-2) of fp64 autograd with
    the same Philox mask.  Switch off: the calls of before (P materialised, a mask tensor, the exact backward)."""
    from oracle import philox_ref
    from snuffy_amd import autograd as SA
    ops = _ops()
    g = torch.Generator().manual_seed(n + k + dk)
    d = h * dk
    q, kp, v, dout = (torch.randn(s, d, generator=g) for s in (n, k, n, k))
    monkeypatch.setattr(SA, "draw_dropout_state", lambda: (SEED, OFFSET))
    rec = _spies(monkeypatch)

    def run():
        for log in rec.values():
            del log[:]
        qd, kd, vd = (t.to(DEV).requires_grad_(True) for t in (q, kp, v))
        out, p = SA.SparseAttnFn.apply(qd, kd, vd, h, P_DROP, True, False)
        saved = [tuple(t.shape) for t in out.grad_fn.saved_tensors if t is not None]
        out.backward(bf16r(dout).to(DEV))
        return out, p, (qd.grad, kd.grad, vd.grad), saved

    monkeypatch.setattr(SA, "SPARSE_ATTN_FN_WIDE", True)
    out, p, grads, saved = run()
    fwd = "sparse_attn_fwd_mfma_dk256" if dk == 256 else "sparse_attn_fwd_mfma"
    assert len(rec[fwd]) == 1 and rec[fwd][0][1]["dropout"] == (P_DROP, SEED, OFFSET)
    assert len(rec["sparse_attn_bwd_mfma"]) == 1 and rec["sparse_attn_bwd_mfma"][0][1]["dropout"] == (P_DROP, SEED, OFFSET)
    assert not rec["dropout_mask"] and not rec["sparse_attn_fwd"] and not rec["sparse_attn_fwd_x3"] and not rec["sparse_attn_bwd"]
    assert p is None and (h, n, k) not in saved and sorted(saved) == sorted([(n, d), (k, d), (n, d), (h, n)])
    mask = torch.from_numpy(philox_ref.dropout_mask(h, n, k, P_DROP, SEED, OFFSET))
    rq, rk, rv, _ = _ref(bf16r(q), bf16r(kp), bf16r(v), bf16r(dout), h, mask)
    print("SparseAttnFn wide dk=%d %s" % (dk, (n, k, h)))
    for got, want, name in zip(grads, (rq, rk, rv), ("dq", "dkp", "dv")):
        _close(got, want, 1.5e-2, name)
    qh, kh, vh = (bf16r(t).double().view(-1, h, dk).transpose(0, 1) for t in (q, kp, v))
    o_r = ((torch.softmax(qh @ kh.transpose(1, 2) / dk ** 0.5, dim=-1) * mask.double()).transpose(1, 2) @ vh).transpose(0, 1).reshape(k, d)
    assert rel_err(out.detach().cpu(), o_r) < 3e-3

    monkeypatch.setattr(SA, "SPARSE_ATTN_FN_WIDE", False)
    out0, _, grads0, saved0 = run()
    assert not rec["sparse_attn_fwd_mfma"] and not rec["sparse_attn_fwd_mfma_dk256"] and not rec["sparse_attn_bwd_mfma"]
    assert len(rec["dropout_mask"]) == 1 and rec["dropout_mask"][0][0][:3] == (h, n, k)
    assert len(rec["sparse_attn_bwd"]) == 1 and len(rec["sparse_attn_fwd"]) + len(rec["sparse_attn_fwd_x3"]) == 1
    assert saved0.count((h, n, k)) == 2                                       # P and the mask tensor
    assert all(bool(torch.isfinite(t).all()) for t in grads0)


@pytest.mark.parametrize("sites", [(0.0, 0.0, 0.0), (0.1, 0.1, 0.1)])
def test_chain_at_dk256_matches_the_restated_layer(sites, monkeypatch):
    """One training step through EncoderLayer0Bf16Fn (asserted by the spy inside _parity) on the D = 512 / h = 2 / Lambda = 900 layer at
    N = 3000 against the plain-torch restatement, with the bounds and the widening rule of tests/test_gpu_encoder_dropout_bf16.py."""
    from snuffy_amd import autograd as SA
    n, d, h, lam = 3000, ROW.D, ROW.H, ROW.LAM
    assert d // h == DK
    monkeypatch.setattr(SA, ROW.train_switch, True)
    _parity(monkeypatch, n, d, h, lam, sites=sites)


def test_stepper_step_takes_the_chain_at_dk256_and_the_switch_takes_it_out(monkeypatch):
    """One optimizer step of the training driver (BagParallelStepper, bf16) on the SimCLR-recipe model: with FUSED_BF16_DK256 on the fused
    chain runs, off it does not; either way the loss is finite and the state_dict keeps its keys and shapes."""
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
