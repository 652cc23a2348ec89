"""Shared test helpers: golden-vector loading, and the operands, fp64 references and comparison rules that several GPU test modules use
(the attention backward's, the encoder-dropout chain's, the model-level gates).  Test modules import from here, never from one another."""
import glob
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda"
BF = torch.bfloat16


def golden_files(prefix):
    return sorted(glob.glob(os.path.join(GOLDEN, prefix + "*.npz")))


def load_case(path, dtype=torch.float32):
    z = np.load(path, allow_pickle=False)
    sd = {k[3:]: torch.from_numpy(z[k]).to(dtype) for k in z.files if k.startswith("sd.")}
    return z, sd


def forced_sel(z, n_layers):
    """Selection per layer as the reference made it: top (same for every layer) + that layer's random draw."""
    top = torch.from_numpy(z["top"].astype(np.int64)) if "top" in z.files else None
    n_rnd = int(z["n_rnd"])
    sels = []
    for l in range(n_layers):
        if n_rnd:
            sels.append(torch.cat([top, torch.from_numpy(z[f"rnd{l}"].astype(np.int64))]))
        else:
            sels.append(top)
    return sels


class ReplayRNG:
    """Stands in for np.random in the oracle: replays MT19937 from a seed (same stream as np.random.seed(seed))."""

    def __init__(self, seed):
        self.rs = np.random.RandomState(seed)

    def permutation(self, n):
        return self.rs.permutation(n)


def build_amd_milnet(D, h, act, big_lambda, r, depth, C=1, mlp=4, enc_drop=0.0):
    """Same construction sequence as the reference's train.Snuffy._get_milnet (train.py:861-890)."""
    from snuffy_amd import snuffy
    return snuffy.build_milnet(D, h, act, big_lambda, r, depth, C, mlp, enc_drop)


def rel_err(a, b):
    """max |a-b| / max |b| (normalised max error)."""
    a = a.double()
    b = b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _ops():
    from snuffy_amd import ops
    return ops


# ---- sparse attention: operands, fp64 references, the backward's C entry points --------------------------------------------------------
def attn_ref(q, kp, v, h):
    from oracle import snuffy_oracle as orc
    o, p = orc.sparse_attention(q.double(), kp.double(), v.double(), h)
    return o, p


def bf16r(t):
    return t.to(BF).float()


def _qv(q, v, dt):
    """Row-strided halves of one [n, 2 d] buffer, as the model passes them."""
    d = q.shape[1]
    qv = torch.cat([q, v], dim=1).to(DEV).to(torch.float32 if dt == "f32" else BF)
    return qv[:, :d], qv[:, d:]


def _c_backward(entry, q, v, kp, dout, lse, h, mask=None, drop=(0.0, 0, 0)):
    """The C entry point itself (fp32 dq / dv; dS in the operands' class, as ops.sparse_attn_bwd_mfma asks for it) -> (dq, dv, ds)."""
    ops = _ops()
    lib = ops._ffi.load()
    n, d = q.shape
    k, dk = kp.shape[0], d // h
    bf = q.dtype == BF
    dq = torch.empty(n, d, dtype=torch.float32, device=DEV)
    dv = torch.empty(n, d, dtype=torch.float32, device=DEV)
    ds = torch.full((h, n, k), float("nan"), dtype=BF if bf else torch.float32, device=DEV)
    head = (ops._p(q), q.stride(0), ops._p(v), v.stride(0), ops.DT_BF16 if bf else ops.DT_F32, ops._p(kp), ops._p(dout), ops._p(lse),
            ops._p(mask), float(drop[0]), int(drop[1]), int(drop[2]), n, k, h, dk, 1.0 / math.sqrt(dk), ops._p(dq), ops._p(dv), d,
            ops.DT_F32, ops._p(ds), ops.DT_BF16 if bf else ops.DT_F32)
    if entry == "chunked":
        wsb = lib.snf_sparse_attn_bwd_mfma_chunked_workspace_bytes(n, k, h, dk, ops.DT_F32)
        ws = ops._ws(wsb, DEV)
        ops.check(lib.snf_sparse_attn_bwd_mfma_chunked(*head, ops._p(ws), wsb, ops._stream()), "snf_sparse_attn_bwd_mfma_chunked")
    else:
        ops.check(lib.snf_sparse_attn_bwd_mfma_ex(*head, ops._stream()), "snf_sparse_attn_bwd_mfma_ex")
    return dq, dv, ds


def _ref(q, kp, v, dout, h, mask):
    """fp64 autograd of O = (softmax(Q Kp^T / sqrt(dk)) o M)^T V -> (dq, dkp, dv, sum_j |P_j dP_j| per head and row)."""
    n, d = q.shape
    k, dk = kp.shape[0], d // h
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, kp, v))
    qh, kh, vh = (t.view(-1, h, dk).transpose(0, 1) for t in (qd, kd, vd))
    p = torch.softmax(qh @ kh.transpose(1, 2) / dk ** 0.5, dim=-1)
    pr = p * mask.double() if mask is not None else p
    (pr.transpose(1, 2) @ vh).transpose(0, 1).reshape(k, d).backward(dout.double())
    with torch.no_grad():
        dp = vh @ dout.double().view(k, h, dk).transpose(0, 1).transpose(1, 2)
        if mask is not None:
            dp = dp * mask.double()
        pdp = (p * dp).abs().sum(-1)
    return qd.grad, kd.grad, vd.grad, pdp


def grad_close(got, want, tol, name):
    """The rule of test_sparse_attn_bwd_mfma: relative to the gradient's own scale."""
    scale_ = max(float(want.abs().max()), 1e-3)
    err = float((got.cpu().double() - want).abs().max())
    print("    %-4s max err %.3e (%.3e of its scale), rel_err %.3e, tol %.1e" % (name, err, err / scale_, rel_err(got.cpu(), want), tol))
    assert err < tol * 4 * scale_ or rel_err(got.cpu(), want) < tol, name


# ---- row passes: the LayerNorm backward in fp64, the split of an fp32 value into bf16 hi / lo ----------------------------------------------
def _ln_reference(x, dy, gamma, eps, residual):
    x = x.double().requires_grad_(True)
    g = gamma.double().requires_grad_(True)
    b = torch.zeros_like(g).requires_grad_(True)
    y = torch.nn.functional.layer_norm(x, (x.shape[1],), g, b, eps)
    y.backward(dy.double().expand_as(y))
    dx = x.grad + (residual.double() if residual is not None else 0)
    return dx, g.grad, b.grad


def _split_host(x):
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return hi, lo


# ---- the encoder layer's training chains against their plain-torch restatement ---------------------------------------------------------
def _perturbed_state_dict(n, d, h, lam):
    torch.manual_seed(n)
    ref = build_amd_milnet(d, h, "relu", lam, 0.0, 1)
    with torch.no_grad():
        for m in ref.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.add_(0.3 * torch.randn(d))
                m.bias.add_(0.2 * torch.randn(d))
            if isinstance(m, torch.nn.Linear) and m.bias is not None:
                m.bias.add_(0.1 * torch.randn_like(m.bias))
    return ref.state_dict()


def _restated_layer(states, arithmetic):
    """EncoderLayer.forward (snuffy.py:126-157) in plain torch under autograd, every dropout as a multiplication by the mask tensor of its
    Philox state.  arithmetic: "library" = fp32 library GEMMs, "x3" = the bag-sized projections through autograd._linear (split-bf16 x 3
    where functional.FP32_GEMM == "x3"), "fp64" = the whole layer in double."""
    from snuffy_amd import autograd as SA
    from snuffy_amd.functional import Parts
    ops = _ops()

    def fn(x2, sel, layer, need_attn, precision):
        mha, ff = layer.self_attn, layer.feed_forward
        n0, n1 = layer.sublayer[0].norm, layer.sublayer[1].norm
        lq, lk, lv, lo = mha.linears
        n, d = x2.shape
        h, k = mha.h, sel.numel()
        dk = d // h
        dt = torch.float64 if arithmetic == "fp64" else torch.float32
        c = lambda t: t.to(dt)

        def big(x, lin):
            if arithmetic == "x3":
                return SA._linear(x, lin)
            return F.linear(x, c(lin.weight), c(lin.bias))

        def mask(site, rows, cols, heads=1):
            st = states[site]
            assert st is not None and st[0] > 0, site
            return c(ops.dropout_mask(heads, rows, cols, st[0], st[1], st[2], x2.device))

        x = c(x2)
        xs = x.index_select(0, sel)
        xn = F.layer_norm(x, (d,), c(n0.weight), c(n0.bias), n0.eps)
        q, v = big(xn, lq), big(xn, lv)
        kp = F.linear(xs, c(lk.weight), c(lk.bias))
        s = torch.einsum("nhd,khd->hnk", q.view(n, h, dk), kp.view(k, h, dk)) / math.sqrt(dk)
        p = torch.softmax(s, dim=-1) * mask("attn", n, k, h)                              # snuffy.py:166-167
        o = torch.einsum("hnk,nhd->khd", p, v.view(n, h, dk)).reshape(k, d)
        delta = F.linear(o, c(lo.weight), c(lo.bias)) * mask("A", k, d)[0]                # snuffy.py:108
        y = x.index_copy(0, sel, xs + delta)
        yn = F.layer_norm(y, (d,), c(n1.weight), c(n1.bias), n1.eps)
        hid = torch.relu(big(yn, ff.w_1)) * mask("H", n, ff.w_1.weight.shape[0])[0]       # snuffy.py:225
        f = big(hid, ff.w_2) * mask("Z", n, d)[0]                                         # snuffy.py:110
        return Parts((y + f).float()), None

    return fn


def _run(monkeypatch, sd, x, d, h, lam, precision, enc_drop=0.1, layer_fn=None, gemm=None, sites=None):
    from snuffy_amd import autograd as SA
    from snuffy_amd import functional as SF
    with monkeypatch.context() as mp:
        if gemm is not None:
            mp.setattr(SF, "FP32_GEMM", gemm)
        if layer_fn is not None:
            mp.setattr(SA, "encoder_layer_train", layer_fn)
        net = build_amd_milnet(d, h, "relu", lam, 0.0, 1, enc_drop=enc_drop)
        net.load_state_dict(sd, strict=True)
        net = net.to(DEV).configure(precision=precision, return_attention=False)
        net.train(True)
        layer = net.b_classifier.encoder.layers[0]
        if sites is not None:
            layer.sublayer[0].dropout.p, layer.feed_forward.dropout.p, layer.sublayer[1].dropout.p = sites
        torch.manual_seed(11)
        np.random.seed(5)
        ins, logits, _ = net(x)
        (logits.sum() * 3 + ins.max()).backward()
        return net, {k: p.grad.float().clone() for k, p in net.named_parameters()}, logits.detach().clone()


def _under_autocast(fn):
    def wrapped(*args):
        with torch.autocast("cuda", torch.bfloat16):
            return fn(*args)
    return wrapped


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-12))


def _parity(monkeypatch, n, d, h, lam, sites=None):
    """The fused bf16 chain against _restated_layer(states, "library") in fp32 (a) and under bf16 autocast (b); bounds of
    test_fused_bf16_layer0_training_matches_generic_and_fp32: logits 2e-2 max(1, |ref|max), gradients 0.08 against (b), 0.1 against (a).
    The distance between (a) and (b) involves no code under test: where it alone exceeds a bound for a key, that key's bound is 1.5 x
    that distance (printed as WIDENED; profiles/encoder_dropout_bf16_train.txt lists them)."""
    from snuffy_amd import autograd as SA
    sd = _perturbed_state_dict(n, d, h, lam)
    x = torch.randn(1, n, d, device=DEV)
    calls = []
    real_apply = SA.EncoderLayer0Bf16Fn.apply
    monkeypatch.setattr(SA.EncoderLayer0Bf16Fn, "apply", lambda *a: (calls.append(1), real_apply(*a))[1])
    enc = 0.1 if sites is None else 0.0
    net, g_fused, out_fused = _run(monkeypatch, sd, x, d, h, lam, "bf16", enc, sites=sites)
    assert calls, "the fused bf16 chain declined a layer with encoder dropout"
    states = dict(net.b_classifier.encoder.layers[0].last_dropout_states)
    want_p = dict(zip(("A", "H", "Z"), sites if sites is not None else (0.1, 0.1, 0.1)))
    assert states["attn"] is not None and states["attn"][0] == 0.1
    for s, p in want_p.items():
        assert (states[s] is None) if p == 0 else (states[s] is not None and states[s][0] == p), (s, states[s])
    drawn = [states[s][2] for s in states if states[s] is not None]
    assert len(set(drawn)) == len(drawn) == 1 + sum(p > 0 for p in want_p.values())       # one Philox offset per site
    # a site that is off: the restatement multiplies by the mask of p = 1e-30, which keeps everything at scale 1.0f
    restate = {s: (st if st is not None else (1e-30, 0, 0)) for s, st in states.items()}
    for s, st in restate.items():
        if states[s] is None:
            assert bool((_ops().dropout_mask(1, 8, 8, *st, DEV) == 1).all())
    del calls[:]
    _, g_a, out_a = _run(monkeypatch, sd, x, d, h, lam, "fp32", enc, _restated_layer(restate, "library"), "library", sites)
    _, g_b, out_b = _run(monkeypatch, sd, x, d, h, lam, "bf16", enc, _under_autocast(_restated_layer(restate, "library")), None, sites)
    assert not calls                                                     # the comparators did not run the chain
    tag = "bf16 encoder dropout parity n=%d d=%d sites=%s" % (n, d, sites)
    for name, out_ref in (("a", out_a), ("b", out_b)):
        err = (out_fused - out_ref).abs().max().item() / max(1.0, out_ref.abs().max().item())
        print("%s: logits vs (%s) %.3e; (a) vs (b) %.3e" % (tag, name, err, (out_a - out_b).abs().max().item() / max(1.0, out_b.abs().max().item())))
        assert err <= 2e-2, (name, err)
    bad = []
    for k in g_fused:
        if k.endswith("self_attn.linears.1.bias"):
            continue                               # mathematically zero gradient
        d_ab = _rel(g_a[k], g_b[k])
        r_a, r_b = _rel(g_fused[k], g_a[k]), _rel(g_fused[k], g_b[k])
        bound_a = 0.1 if d_ab <= 0.1 else 1.5 * d_ab
        bound_b = 0.08 if d_ab <= 0.08 else 1.5 * d_ab
        print("    %-55s vs (a) %.3e  vs (b) %.3e  (a) vs (b) %.3e%s" % (k, r_a, r_b, d_ab, "  WIDENED" if d_ab > 0.08 else ""))
        if not (r_a < bound_a and r_b < bound_b):
            bad.append((k, r_a, bound_a, r_b, bound_b))
    assert not bad, bad


# ---- model-level gates -------------------------------------------------------------------------------------------------------------------
# north-star tolerances: fp32 1e-3, bf16 1e-2 (attention / logits)
TOL = {"fp32": 1e-3, "bf16": 1e-2}


# The gates are FLAT (north_star gives no depth allowance).  precision="bf16" holds 1e-2 for one encoder layer -- the benchmark model;
# stacks of more than one layer run the fp32-class kernels whatever the setting (snuffy.RuntimeConfig.compute): the reference's
# depth-5 fixture f1_n150_d5 measured |dA| = 0.10 through five literal bf16 layers, 1.5e-4 fp32-class.
def tol_for(precision, depth, fixture=None, what="logits"):
    return TOL[precision]


def synth_state(D, h, depth, seed=0):
    """train.py defaults: xavier_normal weights, zero biases (train.py:68-72, utils.py:69-75)."""
    torch.manual_seed(seed)
    net = build_amd_milnet(D, h, "relu", 200, 0.0, depth)
    for _, p in net.named_parameters():
        if p.dim() > 1:
            torch.nn.init.xavier_normal_(p)
    for m in net.modules():
        if isinstance(m, torch.nn.Linear):
            torch.nn.init.zeros_(m.bias)
    return net


# ---- ViT blocks: drawn state dicts, token rows, the exact fp64 blocks ---------------------------------------------------------------------
VIT_EPS = 1e-6
VIT_ROW_KINDS = ("plain", "offset", "outliers")


def vit_block_state(d, depth=1, bott=0, qkv_bias=True, scale_param=None, mlp_ratio=4, seed=0, up_gain=1.0):
    """State dict of `depth` ViT blocks under the reference's key names, nothing at its init value: LayerNorm gamma = 1 + 0.2 randn,
    beta = 0.2 randn, Linear weights randn / sqrt(k), biases 0.2 randn, the adapter's up-projection NON-zero (the LoRA zero init would
    hide the branch).  bott = 0: no adapter.  scale_param: the value of adaptmlp.scale where it is a parameter ("learnable_scalar").
    up_gain multiplies the up-projection: 1 / scalar for a model whose adapter scalar is 10, so that the scaled branch is of the size of
    the MLP's and does not set the scale of the block's update by itself (an error of the other branches would hide behind it)."""
    g = torch.Generator().manual_seed(1000 + seed)

    def lin(sd, name, n, k, bias=True):
        sd[name + ".weight"] = torch.randn(n, k, generator=g) / k ** 0.5
        if bias:
            sd[name + ".bias"] = 0.2 * torch.randn(n, generator=g)

    sd = {}
    for i in range(depth):
        pre = "blocks.%d." % i
        for nm in ("norm1", "norm2"):
            sd[pre + nm + ".weight"] = 1.0 + 0.2 * torch.randn(d, generator=g)
            sd[pre + nm + ".bias"] = 0.2 * torch.randn(d, generator=g)
        lin(sd, pre + "attn.qkv", 3 * d, d, qkv_bias)
        lin(sd, pre + "attn.proj", d, d)
        lin(sd, pre + "mlp.fc1", mlp_ratio * d, d)
        lin(sd, pre + "mlp.fc2", d, mlp_ratio * d)
        if bott:
            if scale_param is not None:
                sd[pre + "adaptmlp.scale"] = torch.tensor([float(scale_param)])
            lin(sd, pre + "adaptmlp.down_proj", bott, d)
            lin(sd, pre + "adaptmlp.up_proj", d, bott)
            sd[pre + "adaptmlp.up_proj.weight"] *= up_gain
            sd[pre + "adaptmlp.up_proj.bias"] *= up_gain
    return sd


def vit_token_rows(kind, rows, d, seed=0):
    """Token matrix [rows, d] f32.  plain: randn; offset: randn + 4 (sign alternating by row: |row mean| = 4 row spreads); outliers:
    randn with channel 5 = +150 and channel 77 = -60 in every row (two massive activations, row mean ~ 0)."""
    g = torch.Generator().manual_seed(2000 + seed)
    x = torch.randn(rows, d, generator=g)
    if kind == "offset":
        x += 4.0 * (1.0 - 2.0 * (torch.arange(rows) % 2)).unsqueeze(1)
    elif kind == "outliers":
        x[:, 5], x[:, 77] = 150.0, -60.0
    elif kind != "plain":
        raise ValueError(kind)
    return x


def vit_blocks_update_fp64(x, sd, b, t, heads, depth, adapter_scale, images_per_pass=8):
    """blocks(x) - x in float64 for the token matrix x [b * t, d]: oracle.vit_oracle.block over the drawn state dict, a few images at a
    time (images do not interact; the [B, h, T, T] probabilities of all of them at once would not fit at T = 785)."""
    from oracle import vit_oracle as vorc
    sd64 = {k: v.double() for k, v in sd.items()}
    x3 = x.double().view(b, t, -1)
    out = torch.empty_like(x3)
    for i in range(0, b, images_per_pass):
        y = x3[i:i + images_per_pass]
        for j in range(depth):
            y = vorc.block(y, sd64, "blocks.%d." % j, heads, adapter_scale, VIT_EPS)
        out[i:i + images_per_pass] = y
    return (out - x3).view(b * t, -1)
