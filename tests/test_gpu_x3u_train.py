"""fp32-class training attention at the head widths outside the pipelined x 3 kernels (dk = 96 / 192 / 256: the README's DINO, MAE and
SimCLR recipes): the dropout form of the unfused pair (snf_sparse_attn_fwd_x3u_dropout_f32: split-bf16 x 3 scores + softmax, then the
LDS pooling pass with the Philox mask regenerated in registers), the exact backward regenerating the same mask at these widths, and the
routing of autograd.SparseAttnFn / EncoderLayer0X3Fn behind autograd.X3U_TRAINING, switch on against switch off."""
import numpy as np
import pytest
import torch

from oracle import philox_ref
from tests.helpers import DEV, _ref, _rel, build_amd_milnet, rel_err

pytestmark = pytest.mark.gpu

# (n, k, h, dk, p): smallest | a one-row tail after a full chunk, two heads | two row slices (304 + 296 rows, half-chunk tails), a second
# key tile of 4 keys, two column groups | SimCLR recipe: four key tiles, CT = 4 | MAE recipe | DINO recipe: one column group | the key
# limit | one column block
SHAPES = [(1, 4, 1, 192, 0.1), (33, 8, 2, 256, 0.5), (600, 260, 2, 192, 0.1), (1000, 900, 2, 256, 0.1), (700, 500, 4, 192, 0.1),
          (515, 300, 4, 96, 0.25), (130, 1024, 1, 256, 0.1), (520, 36, 3, 16, 0.1)]


def _ops():
    from snuffy_amd import ops
    return ops


def _state(n, k):
    return 1234567 + n, (1 << 40) + 17 * k


def _operands(n, k, h, dk):
    g = torch.Generator().manual_seed(n + k + dk)
    d = h * dk
    return tuple(torch.randn(s, d, generator=g).to(DEV) for s in (n, k, n))


@pytest.mark.parametrize("n,k,h,dk,p_drop", SHAPES)
def test_x3u_in_kernel_dropout(n, k, h, dk, p_drop):
    """O = (P o M)^T V with M regenerated in the pooling pass, against the host Philox mask (oracle/philox_ref.py) applied to the kernel's
    own undropped P in fp64: 2e-5 (the bound of test_sparse_attn_x3_in_kernel_dropout).  attn / lse are the plain launch's bit for bit, a
    repeat call and the row-strided halves of one [n, 2 d] buffer give the same bits, p = 0 is the plain call."""
    ops = _ops()
    d = h * dk
    q, kp, v = _operands(n, k, h, dk)
    seed, offset = _state(n, k)
    drop = (p_drop, seed, offset)
    mask = torch.from_numpy(philox_ref.dropout_mask(h, n, k, p_drop, seed, offset))
    assert float(mask.max()) > 0                                       # at least one key kept: rel_err's denominator is not zero
    kept = (mask > 0).float().mean().item()
    assert abs(kept - (1 - p_drop)) < 0.02 + 2.0 / (h * n * k) ** 0.5
    assert ops.x3u_attn_dropout_supported(k, dk)
    o_plain, p_plain, lse_plain = ops.sparse_attn_fwd_x3u(q, kp, v, h, need_attn=True, need_lse=True)
    o, p, lse = ops.sparse_attn_fwd_x3u(q, kp, v, h, need_attn=True, need_lse=True, dropout=drop)
    assert torch.equal(p, p_plain) and torch.equal(lse, lse_plain)
    assert torch.equal(ops.dropout_mask(h, n, k, p_drop, seed, offset, DEV).cpu(), mask)
    ref = torch.bmm((p.cpu().double() * mask.double()).transpose(1, 2),
                    v.cpu().double().view(n, h, dk).transpose(0, 1)).transpose(0, 1).reshape(k, d)
    err = rel_err(o.cpu(), ref)
    print("x3u dropout n=%d k=%d h=%d dk=%d p=%.2f: rel_err %.3e (bound 2e-5), kept %.4f" % (n, k, h, dk, p_drop, err, kept))
    assert err < 2e-5
    if h * n * k >= 10 ** 5:
        assert rel_err(o.cpu(), o_plain.cpu()) > 1e-3                  # and it is not the undropped product
    o2, p2, _ = ops.sparse_attn_fwd_x3u(q, kp, v, h, need_attn=True, dropout=drop)
    assert torch.equal(o2, o) and torch.equal(p2, p)
    o0, p0, _ = ops.sparse_attn_fwd_x3u(q, kp, v, h, need_attn=True, dropout=(0.0, seed, offset))
    assert torch.equal(o0, o_plain) and torch.equal(p0, p_plain)
    qv = torch.cat([q, v], dim=1)
    o3, p3, _ = ops.sparse_attn_fwd_x3u(qv[:, :d], kp, qv[:, d:], h, need_attn=True, dropout=drop)
    assert torch.equal(o3, o) and torch.equal(p3, p)


def test_x3u_dropout_refusals():
    from snuffy_amd import SnuffyHipError
    ops = _ops()
    q, kp, v = _operands(64, 901, 2, 256)
    with pytest.raises(SnuffyHipError):                                # k % 4 != 0: no LDS pooling pass, no dropout form
        ops.sparse_attn_fwd_x3u(q, kp, v, 2, need_attn=True, dropout=(0.1, 1, 2))
    with pytest.raises(SnuffyHipError):
        ops.sparse_attn_fwd_x3u(q, kp[:900].contiguous(), v, 2, need_attn=True, dropout=(1.0, 1, 2))
    with pytest.raises(ValueError):                                    # the undropped P has to go somewhere
        ops.sparse_attn_fwd_x3u(q, kp[:900].contiguous(), v, 2, dropout=(0.1, 1, 2))


@pytest.mark.parametrize("n,k,h,dk", [(600, 260, 2, 192), (1000, 900, 2, 256)])
def test_exact_backward_regenerates_the_mask_at_the_wide_widths(n, k, h, dk):
    """snf_sparse_attn_bwd_dropout_f32 at dk = 192 / 256: bit for bit the backward that reads the mask tensor, and both within 2e-5 of fp64
    autograd with that mask (the bound and formulation of test_sparse_attn_bwd_matches_autograd_reference)."""
    ops = _ops()
    q, kp, v = _operands(n, k, h, dk)
    dout = torch.randn(k, h * dk, generator=torch.Generator().manual_seed(n)).to(DEV)
    seed, offset = _state(n, k)
    drop = (0.1, seed, offset)
    assert ops.attn_bwd_dropout_supported(k, dk)
    _, p, _ = ops.sparse_attn_fwd(q, kp, v, h, need_attn=True)
    mask = ops.dropout_mask(h, n, k, *drop, DEV)
    regen = ops.sparse_attn_bwd(q, kp, v, p, dout, h, dropout=drop)
    tensor = ops.sparse_attn_bwd(q, kp, v, p, dout, h, mask=mask)
    want = _ref(q.cpu(), kp.cpu(), v.cpu(), dout.cpu(), h, mask.cpu())[:3]
    for a, b, w, name in zip(regen, tensor, want, ("dq", "dkp", "dv")):
        assert torch.equal(a, b), name
        err = rel_err(a.cpu(), w)
        print("exact backward n=%d k=%d dk=%d %s: rel_err %.3e (bound 2e-5)" % (n, k, dk, name, err))
        assert err < 2e-5, name


# ---- model level: switch on against switch off ------------------------------------------------------------------------------------------
MODELS = {
    "generic": dict(d=512, h=2, lam=900, share=7 / 9, act="gelu", depth=2, n=1200),     # SparseAttnFn in every layer
    "fused192": dict(d=768, h=4, lam=500, share=0.5, act="relu", depth=1, n=1024),      # EncoderLayer0X3Fn at dk = 192
    "fused96": dict(d=384, h=4, lam=300, share=0.5, act="relu", depth=1, n=1024),       # ... and at dk = 96
}
GATE_KEYS = ("feed_forward.w_1.weight", "feed_forward.w_1.bias", "sublayer.1.norm.weight", "sublayer.1.norm.bias")
SMALL_KEYS = ("linears.0.weight", "linears.0.bias", "linears.1.weight", "sublayer.0.norm.weight")


def _state_dict(cfg):
    torch.manual_seed(cfg["n"])
    ref = build_amd_milnet(cfg["d"], cfg["h"], cfg["act"], cfg["lam"], cfg["share"], cfg["depth"])
    with torch.no_grad():
        for m in ref.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.add_(0.3 * torch.randn(cfg["d"]))
                m.bias.add_(0.2 * torch.randn(cfg["d"]))
            if isinstance(m, torch.nn.Linear) and m.bias is not None:
                m.bias.add_(0.1 * torch.randn_like(m.bias))
    return ref.state_dict()


def _step(monkeypatch, cfg, sd, x, on, train_mode, gemm="x3", return_attention=False):
    """One forward + backward; (net, gradients, logits, A, calls of EncoderLayer0X3Fn)."""
    from snuffy_amd import autograd as SA
    from snuffy_amd import functional as SF
    with monkeypatch.context() as mp:
        mp.setattr(SA, "X3U_TRAINING", on)
        mp.setattr(SF, "FP32_GEMM", gemm)
        calls = []
        real_apply = SA.EncoderLayer0X3Fn.apply
        mp.setattr(SA.EncoderLayer0X3Fn, "apply", lambda *a: (calls.append(1), real_apply(*a))[1])
        net = build_amd_milnet(cfg["d"], cfg["h"], cfg["act"], cfg["lam"], cfg["share"], cfg["depth"])
        net.load_state_dict(sd, strict=True)
        net = net.to(DEV).configure(precision="fp32", return_attention=return_attention)
        net.train(train_mode)
        torch.manual_seed(11)
        np.random.seed(5)
        ins, logits, attn = net(x)
        (logits.sum() * 3 + ins.max()).backward()
        grads = {k: p.grad.float().clone() for k, p in net.named_parameters()}
        return net, grads, logits.detach().clone(), attn, len(calls)


def _bound(key):
    return 5e-3 if key.endswith(SMALL_KEYS) else 3e-3 if key.endswith(GATE_KEYS) else 5e-4


def _compare(monkeypatch, cfg, sd, x, train_mode, tag):
    """Switch on against switch off with the bounds of test_fused_x3_layer0_training_matches_the_generic_fp32_chain: logits 5e-5
    max(1, |ref|), gradients by relative norm 5e-4 / 5e-3 (its small_keys) / 3e-3 (its gate_keys).  A key that misses its bound gets the
    rule of tests/helpers._parity: the same distance between two switch-off runs that differ only in FP32_GEMM ("x3" / "library", no code
    under test) is measured and the key's bound becomes 1.5 x that distance."""
    _, g_on, out_on, _, calls_on = _step(monkeypatch, cfg, sd, x, True, train_mode)
    _, g_off, out_off, _, calls_off = _step(monkeypatch, cfg, sd, x, False, train_mode)
    assert calls_on == calls_off
    err = (out_on - out_off).abs().max().item() / max(1.0, out_off.abs().max().item())
    print("%s: logits on vs off %.3e (bound 5e-5)" % (tag, err))
    assert err <= 5e-5
    rels = {k: _rel(g_on[k], g_off[k]) for k in g_on if not k.endswith("self_attn.linears.1.bias")}      # (mathematically zero gradient)
    for k, r in rels.items():
        print("    %-55s %.3e (bound %.0e)" % (k, r, _bound(k)))
    missed = [k for k, r in rels.items() if not r < _bound(k)]
    if missed:
        _, g_lib, _, _, _ = _step(monkeypatch, cfg, sd, x, False, train_mode, gemm="library")
        bad = []
        for k in missed:
            d_lib = _rel(g_off[k], g_lib[k])
            print("    WIDENED %-47s on vs off %.3e, x3 vs library (both off) %.3e" % (k, rels[k], d_lib))
            if not rels[k] < 1.5 * d_lib:
                bad.append((k, rels[k], _bound(k), 1.5 * d_lib))
        assert not bad, bad
    return calls_on


@pytest.mark.parametrize("train_mode", [True, False])
@pytest.mark.parametrize("case", sorted(MODELS))
def test_training_step_switch_on_matches_switch_off(case, train_mode, monkeypatch):
    """Train mode: both runs draw the same Philox states (on: the mask regenerated in the pooling pass and in the backward; off: the mask
    tensor and torch.bmm).  Eval mode: p = 0, the pair against the exact forward."""
    cfg = MODELS[case]
    sd = _state_dict(cfg)
    x = torch.randn(1, cfg["n"], cfg["d"], device=DEV)
    calls = _compare(monkeypatch, cfg, sd, x, train_mode, "%s train=%s" % (case, train_mode))
    assert calls == (0 if case == "generic" else 1)                   # fused_layer0_x3_ok held for the two ReLU models, not for GELU


def test_short_bag_with_odd_k_keeps_the_mask_tensor(monkeypatch):
    """N = 301 < Lambda = 900: K = 301, no dropout form of the pooling pass -- the forward is still the pair, the mask tensor and the bmm
    stay, and the step is within the same bounds of the switch-off run."""
    ops = _ops()
    cfg = dict(MODELS["generic"], n=301)
    sd = _state_dict(cfg)
    x = torch.randn(1, cfg["n"], cfg["d"], device=DEV)
    seen = []
    real = ops.sparse_attn_fwd_x3u
    monkeypatch.setattr(ops, "sparse_attn_fwd_x3u", lambda *a, **kw: (seen.append((a[1].shape[0], kw.get("dropout"))), real(*a, **kw))[1])
    _compare(monkeypatch, cfg, sd, x, True, "short bag")
    assert len(seen) == cfg["depth"] and all(k == 301 and drop is None for k, drop in seen), seen


def test_no_mask_tensor_and_no_bmm_with_the_switch_on(monkeypatch):
    """return_attention off: one training step of the generic case writes no mask tensor and recomputes no O."""
    ops = _ops()
    cfg = MODELS["generic"]
    sd = _state_dict(cfg)
    x = torch.randn(1, cfg["n"], cfg["d"], device=DEV)

    real_bmm = torch.bmm

    def refuse(*a, **kw):
        raise AssertionError("the mask tensor of the routing before")

    def refuse_pooling(a, *rest, **kw):
        # (P o M)^T [h, K, N] against V: the recomputed O.  The weight-gradient contractions may batch over row chunks with bmm: not meant
        if a.dim() == 3 and a.shape[0] == cfg["h"] and a.shape[2] == cfg["n"]:
            raise AssertionError("the bmm of the routing before")
        return real_bmm(a, *rest, **kw)

    with monkeypatch.context() as mp:
        mp.setattr(ops, "dropout_mask", refuse)
        mp.setattr(torch, "bmm", refuse_pooling)
        _, grads, logits, _, _ = _step(monkeypatch, cfg, sd, x, True, True)
    assert bool(torch.isfinite(logits).all()) and all(bool(torch.isfinite(g).all()) for g in grads.values())


def test_return_attention_gets_the_dropped_p(monkeypatch):
    """The caller asked for A: the mask tensor is written (ops.dropout_mask) and A is the pair's undropped P times that mask, bit for bit."""
    ops = _ops()
    cfg = MODELS["generic"]
    sd = _state_dict(cfg)
    x = torch.randn(1, cfg["n"], cfg["d"], device=DEV)
    masks, ps = [], []
    real_mask, real_fwd = ops.dropout_mask, ops.sparse_attn_fwd_x3u
    monkeypatch.setattr(ops, "dropout_mask", lambda *a, **kw: (masks.append(real_mask(*a, **kw)), masks[-1])[1])
    monkeypatch.setattr(ops, "sparse_attn_fwd_x3u", lambda *a, **kw: (ps.append(real_fwd(*a, **kw)), ps[-1])[1])
    _, _, _, attn, _ = _step(monkeypatch, cfg, sd, x, True, True, return_attention=True)
    assert len(ps) == cfg["depth"] and len(masks) == 1                 # only the last layer returns its A
    assert attn is not None and torch.equal(attn.reshape(ps[-1][1].shape), ps[-1][1] * masks[0])
