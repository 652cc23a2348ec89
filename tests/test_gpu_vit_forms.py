"""ViT extractor, the places tests/test_gpu_vit.py leaves open: the fp32-class block at every format state `vit.image_format` can pick
(all "cat", qkv / fc1 "hl" next to proj / fc2 "cat", all "hl" at T = 197 and at T = 785 -- row counts that fill the chip, which no other
test reaches), the bf16 blocks (fused and round-2) over ALL token rows and every form the shapes select, and the arithmetic envelope of
the LayerNorm fold (vit_row_stats + gemm_bf16_lnfold) against the ratio r = |row mean| / row spread.

The oracle is oracle.vit_oracle.block in float64 on the CPU, over a state dict the test draws (tests/helpers.vit_block_state: nothing at
its init value, adapter up-projection non-zero).  Sections 1 and 2 compare the blocks' UPDATE y - x_in over all rows (the residual is
carried in fp32: comparing y would let |x| set the scale), rel_err against the fp64 update, on three kinds of token rows
(helpers.vit_token_rows: plain, offset = mean 4 spreads, outliers = two massive channels).

Bounds of sections 1 and 2 (profiles/vit_blocks.txt has every figure): 4 x the largest value measured in the class, under a cap set
beforehand from the project's gates -- fp32-class 2e-4 (the block0 atol of test_vit_models_match_reference_goldens under x3), library
GEMMs 5e-5, bf16 1e-2 (the flat gate).

Bounds of section 3 are set by the reference: the statistics' by the number format (two-pass rstd 1e-5; one-pass rstd from the moment
pairs 16 (1 + r^2) 2^-24, the cancellation in s2 / d - mean^2), the fold's output by the error e_u of the unfused recipe (LayerNorm in
fp32, rounded to bf16, times the bf16 weight, accumulated in fp64 IN THE TEST on the same operands): at most 1.5 sqrt(1 + r^2) e_u, plus
2^-9 of the output scale for the rounding of the kernel's bf16 result.  That last term is not in the arithmetic's envelope: e_u is an
fp64 product, the kernel returns bf16, and half a bf16 ulp of the largest outputs is 2^-9 in rel_err's units.  Without it the r = 0 case
cannot hold for any kernel that returns bf16: measured at d = 192 the kernel is at 3.91e-3, the same arithmetic with an fp64 result at
2.28e-3 = 0.93 e_u, 1.5 e_u = 3.67e-3 (d = 384: 3.69e-3 / 2.48e-3 / 3.80e-3).  From r = 1 up the kernel is inside 1.5 sqrt(1 + r^2) e_u
by itself (largest ratio 1.30 at r = 1, 0.7 - 0.9 from r = 4); every figure is printed and kept in profiles/vit_blocks.txt."""
import math
from functools import partial

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import VIT_EPS, rel_err, vit_block_state, vit_blocks_update_fp64, vit_token_rows

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
LN = partial(torch.nn.LayerNorm, eps=VIT_EPS)

# 4 x the largest measured value of the class (profiles/vit_blocks.txt), never above the cap
CAP_X3, CAP_LIBRARY, CAP_BF16 = 2e-4, 5e-5, 1e-2
BOUND_X3 = min(CAP_X3, 4 * 1.496e-5)            # hl, adapter 32 x 10, outlier rows
BOUND_LIBRARY = min(CAP_LIBRARY, 4 * 1.678e-6)  # hl, outlier rows
BOUND_BF16 = min(CAP_BF16, 4 * 8.641e-3)        # d384_t5_b53_ad64_offset, fused: the cap binds


def _cus():
    from snuffy_amd import _ffi
    return _ffi.load().snf_device_cu_count()


# -- 1. fp32-class block at the format states -------------------------------------------------------------------------------------
D1, H1 = 384, 6
# state: (T, formats wanted for (qkv, proj, fc1, fc2, up-proj))
STATES = {
    "cat": (197, ("cat", "cat", "cat", "cat", "cat")),
    "mixed": (197, ("hl", "cat", "hl", "cat", "cat")),
    "hl": (197, ("hl", "hl", "hl", "hl", "hl")),
    "hl_t785": (785, ("hl", "hl", "hl", "hl", "hl")),
}
# form: (bottleneck, adapter scalar, qkv bias, FP32_GEMM)
FORMS = {
    "ad32_s10": (32, "10", True, "x3"),
    "ad64": (64, "0.1", True, "x3"),
    "none": (0, "0.1", True, "x3"),
    "learnable": (64, "learnable_scalar", True, "x3"),
    "nobias": (32, "10", False, "x3"),
    "library": (32, "10", True, "library"),
}
LEARNED_SCALE = 0.7
# per state: the DINO recipe's form on every kind of rows, every other form on one; "library" follows the case whose reference it shares
FORM_CASES = [("ad32_s10", "plain"), ("ad32_s10", "offset"), ("ad32_s10", "outliers"), ("library", "outliers"), ("ad64", "offset"),
              ("none", "outliers"), ("learnable", "plain"), ("nobias", "offset")]
_BLOCKS, _LAST_REF = {}, {}


def state_batch(state, cus):
    """(B, T) of a format state on a chip of `cus` CUs: ops.hl_eligible wants ceil(m / 256) ceil(n / 256) 10 >= 7 cus, so the first
    batch whose rows give qkv (n = 1152, 5 column tiles) that many tiles is the mixed state, the first that gives them to the n = 384
    projections (2 column tiles) the all-"hl" one.  256 CUs: B = 4 / 46 / 116 at T = 197, 30 at T = 785."""
    t = STATES[state][0]
    if state == "cat":
        return 4, t
    col_tiles = (3 * D1 + 255) // 256 if state == "mixed" else (D1 + 255) // 256
    row_tiles = -(-7 * cus // (10 * col_tiles))
    return -(-((row_tiles - 1) * 256 + 1) // t), t


def test_state_batches_at_256_cus():
    assert [state_batch(s, 256) for s in STATES] == [(4, 197), (46, 197), (116, 197), (30, 785)]
    assert 116 * 197 % 256 and 30 * 785 % 256                       # ragged last row tile


def _block(form):
    from snuffy_amd import vit
    if form not in _BLOCKS:
        bott, scalar, qkv_bias, _ = FORMS[form]
        learn = scalar == "learnable_scalar"
        scale = LEARNED_SCALE if learn else float(scalar)
        sd = vit_block_state(D1, 1, bott, qkv_bias, LEARNED_SCALE if learn else None, seed=bott + 7 * qkv_bias,
                             up_gain=1 / max(1.0, scale))
        blk = vit.Block(D1, H1, 4.0, qkv_bias=qkv_bias, norm_layer=LN, adapter_ffn_scalar=scalar, adapter_ffn_num=bott or 64,
                        d_model=D1, adapter_d_model=D1, use_adapter=bott > 0)
        blk.load_state_dict({k[len("blocks.0."):]: v for k, v in sd.items()}, strict=True)
        _BLOCKS[form] = (blk.to(DEV).eval(), sd, scale)
    return _BLOCKS[form]


def _reference(key, fn):
    """One reference is alive at a time (an update is 70 MB at the chip-filling states); neighbours in FORM_CASES share theirs."""
    if _LAST_REF.get("key") != key:
        _LAST_REF.clear()
        _LAST_REF.update(key=key, value=fn())
    return _LAST_REF["value"]


class Launches:
    """Counts what a block launches (the module attributes vit.py calls through)."""
    NAMES = ("gemm_hl", "gemm_x3", "vit_attention", "layernorm_rows_hl", "layernorm_rows_split3")

    def __init__(self, monkeypatch):
        from snuffy_amd import ops
        self.calls = []
        for name in self.NAMES:
            real = getattr(ops, name)
            monkeypatch.setattr(ops, name, lambda *a, _n=name, _f=real, **kw: (self.calls.append((_n, kw)), _f(*a, **kw))[1])

    def count(self, name, resid=None, hl_out=None):
        """Calls of `name`; resid / hl_out (True / False): only those that did / did not pass a residual / ask for an hl image."""
        hits = [kw for n, kw in self.calls if n == name]
        if resid is not None:
            hits = [kw for kw in hits if (kw.get("resid") is not None) == resid]
        if hl_out is not None:
            hits = [kw for kw in hits if bool(kw.get("hl_out", False)) == hl_out]
        return len(hits)


@pytest.mark.parametrize("form,kind", FORM_CASES, ids=["%s-%s" % c for c in FORM_CASES])
@pytest.mark.parametrize("state", list(STATES))
def test_fp32_block_update_at_format_state(state, form, kind, monkeypatch):
    from snuffy_amd import vit
    bott, scalar, qkv_bias, gemm = FORMS[form]
    monkeypatch.setattr(vit, "FP32_GEMM", gemm)
    b, t = state_batch(state, _cus())
    m = b * t
    blk, sd, scale = _block(form)
    weights = [blk.attn.qkv.weight, blk.attn.proj.weight, blk.mlp.fc1.weight, blk.mlp.fc2.weight]
    weights += [blk.adaptmlp.up_proj.weight] if bott else []
    want = STATES[state][1][:len(weights)] if gemm == "x3" else (None,) * len(weights)
    # before anything runs: on another CU count the case must fail here, not pass through another kernel
    assert tuple(vit.image_format(m, w) for w in weights) == want, (state, b, t, _cus())
    x = vit_token_rows(kind, m, D1, seed=STATES[state][0] + b)
    ref = _reference((state, bott, qkv_bias, scale, kind), lambda: vit_blocks_update_fp64(x, sd, b, t, H1, 1, scale))
    seen = Launches(monkeypatch)
    with torch.no_grad():
        y = blk(x.to(DEV).view(b, t, D1))
    assert y.dtype == torch.float32 and tuple(y.shape) == (b, t, D1)
    upd = y.cpu().view(m, D1).double() - x.double()
    e = rel_err(upd, ref)
    e_tail = rel_err(upd[-(m % 256 or 256):], ref[-(m % 256 or 256):])
    print("MEASURED vit fp32 block %-8s %-9s %-8s rows %5d  update rel_err %.3e  last row tile %.3e  (|update| max %.2f)"
          % (state, form, kind, m, e, e_tail, float(ref.abs().max())))
    assert e < (BOUND_X3 if gemm == "x3" else BOUND_LIBRARY)
    # ... through the kernels the state stands for
    folded_adapter = bott > 0 and scalar != "learnable_scalar"
    if gemm != "x3":
        assert not seen.count("gemm_hl") and not seen.count("gemm_x3")
    elif state in ("hl", "hl_t785"):
        assert seen.count("layernorm_rows_hl") == 2 and seen.count("vit_attention", hl_out=True) == 1
        assert seen.count("gemm_hl", resid=True) == 2 + folded_adapter and seen.count("gemm_hl", hl_out=True) == 1
        assert seen.count("gemm_x3") == (bott > 0)                    # the adapter's down-projection: n < 256 never fills the chip
    elif state == "mixed":
        assert seen.count("layernorm_rows_hl") == 2 and seen.count("vit_attention", hl_out=True) == 0
        assert seen.count("gemm_hl") == 2 and seen.count("gemm_hl", resid=True) == 0 and seen.count("gemm_x3") == 2 + 2 * (bott > 0)
    else:
        assert seen.count("gemm_hl") == 0 and seen.count("layernorm_rows_split3") == 2 and seen.count("gemm_x3") == 4 + 2 * (bott > 0)


# -- 2. bf16 blocks, all rows -----------------------------------------------------------------------------------------------------
# name: (D, heads, T, B, depth, bottleneck, qkv bias, BF16_FUSED_BLOCK, row kind, fused path expected)
BF16_CASES = {
    "d384_t197_b3_ad32_plain": (384, 6, 197, 3, 1, 32, True, True, "plain", True),
    "d384_t197_b3_ad32_offset": (384, 6, 197, 3, 1, 32, True, True, "offset", True),
    "d384_t197_b3_ad32_outliers": (384, 6, 197, 3, 1, 32, True, True, "outliers", True),
    "d384_t197_b3_depth2_ad32_plain": (384, 6, 197, 3, 2, 32, True, True, "plain", True),
    "d384_t197_b1_depth2_ad64_offset": (384, 6, 197, 1, 2, 64, True, True, "offset", True),          # 197 rows: one cut tile
    "d384_t197_b3_none_outliers": (384, 6, 197, 3, 1, 0, True, True, "outliers", True),
    "d384_t197_b3_nobias_plain": (384, 6, 197, 3, 1, 32, False, True, "plain", True),
    "d384_t197_b3_ad80_plain": (384, 6, 197, 3, 1, 80, True, True, "plain", False),                  # K = 1536 + 80 leaves the fused domain
    "d384_t5_b3_depth2_ad32_plain": (384, 6, 5, 3, 2, 32, True, True, "plain", True),                # 15 rows
    "d384_t5_b53_ad64_offset": (384, 6, 5, 53, 1, 64, True, True, "offset", True),                   # 265 rows: 9 in the second tile
    "d384_t785_b1_ad32_plain": (384, 6, 785, 1, 1, 32, True, True, "plain", True),                   # keys in LDS chunks
    "d384_t785_b2_depth2_none_outliers": (384, 6, 785, 2, 2, 0, True, True, "outliers", True),
    "d192_t197_b3_depth2_ad32_offset": (192, 3, 197, 3, 2, 32, True, True, "offset", True),
    "d192_t5_b53_none_plain": (192, 3, 5, 53, 1, 0, True, True, "plain", True),
    "d192_t785_b1_ad64_outliers": (192, 3, 785, 1, 1, 64, True, True, "outliers", True),
    "d256_h2_t197_b2_ad32_plain": (256, 2, 197, 2, 1, 32, True, True, "plain", False),               # dk = 128: exact attention
    "unfused_d384_t197_b3_depth2_ad32_plain": (384, 6, 197, 3, 2, 32, True, False, "plain", False),
    "unfused_d384_t197_b3_ad32_offset": (384, 6, 197, 3, 1, 32, True, False, "offset", False),
    "unfused_d384_t197_b3_ad32_outliers": (384, 6, 197, 3, 1, 32, True, False, "outliers", False),
    "unfused_d192_t5_b53_none_plain": (192, 3, 5, 53, 1, 0, True, False, "plain", False),
    "unfused_d384_t785_b1_ad64_offset": (384, 6, 785, 1, 1, 64, True, False, "offset", False),
    "unfused_d384_t5_b3_nobias_outliers": (384, 6, 5, 3, 1, 32, False, False, "outliers", False),
}
BF16_SCALARS = {0: "0.1", 32: "10", 64: "0.1", 80: "1.0"}
_MODELS = {}


def _model(d, heads, depth, bott, qkv_bias, img=32, patch=16, pool="cls"):
    from snuffy_amd import vit
    key = (d, heads, depth, bott, qkv_bias, img, patch, pool)
    if key not in _MODELS:
        torch.manual_seed(3)
        sd = vit_block_state(d, depth, bott, qkv_bias, seed=d + depth + bott + 7 * qkv_bias,
                             up_gain=1 / max(1.0, float(BF16_SCALARS[bott])))
        model = vit.VisionTransformer(img_size=[img], patch_size=patch, embed_dim=d, depth=depth, num_heads=heads, mlp_ratio=4,
                                      qkv_bias=qkv_bias, norm_layer=LN, adapter_ffn_scalar=BF16_SCALARS[bott],
                                      adapter_ffn_num=bott or 64, adapter_d_model=d, use_adapter=bott > 0, pool=pool)
        res = model.load_state_dict(sd, strict=False)
        assert not res.unexpected_keys and not [k for k in res.missing_keys if k.startswith("blocks.")]
        _MODELS[key] = (model.to(DEV).eval().configure("bf16"), sd)
    return _MODELS[key]


def _run_blocks(model, x, b, t, fused):
    xt = x.to(DEV).clone()
    with torch.no_grad():
        run = model._blocks_fused if fused else model._blocks_unfused
        pooled = run(xt, model._weights_bf16(), b, t)
    return xt, pooled


@pytest.mark.parametrize("name", list(BF16_CASES))
def test_bf16_blocks_update_all_rows(name, monkeypatch):
    from snuffy_amd import ops, vit
    d, heads, t, b, depth, bott, qkv_bias, flag, kind, want_fused = BF16_CASES[name]
    monkeypatch.setattr(vit, "BF16_FUSED_BLOCK", flag)
    model, sd = _model(d, heads, depth, bott, qkv_bias)
    m = b * t
    # which path forward_cols takes for this case
    mfma = ops.vit_mfma_attention_supported(t, d // heads)
    assert mfma == (d // heads == 64)
    assert model._fused_ok() == (bott != 80)
    assert (vit.BF16_FUSED_BLOCK and mfma and model._fused_ok()) == want_fused
    x = vit_token_rows(kind, m, d, seed=m + d)
    ref = vit_blocks_update_fp64(x, sd, b, t, heads, depth, float(BF16_SCALARS[bott]))
    if want_fused:
        # the fold's identity is exact only with the column sums of the ROUNDED product (a constant row must give bias alone)
        for wb in model._weights_bf16()["blocks"]:
            for tag in ("qkv", "fc1"):
                assert torch.equal(wb[tag + "_cs"], wb[tag + "_wf"].double().sum(1).float())
    xt, pooled = _run_blocks(model, x, b, t, want_fused)
    assert xt.dtype == torch.float32 and tuple(pooled.shape) == (b, d)
    upd = xt.cpu().double() - x.double()
    e = rel_err(upd, ref)
    tail = m % 256 or 256
    e_tail = rel_err(upd[-tail:], ref[-tail:])
    worst = int((upd - ref).abs().amax(1).argmax())
    print("MEASURED vit bf16 blocks %-40s %-7s rows %4d  update rel_err %.3e  last row tile %.3e  worst row %d (|update| max %.2f)"
          % (name, "fused" if want_fused else "round-2", m, e, e_tail, worst, float(ref.abs().max())))
    assert e < BOUND_BF16
    # the pooled output is LayerNorm of the CLS rows of that stream
    gamma, beta = (p.detach().cpu().double() for p in (model.norm.weight, model.norm.bias))
    want = F.layer_norm(xt.view(b, t, d)[:, 0].cpu().double(), (d,), gamma, beta, VIT_EPS)
    assert rel_err(pooled.cpu(), want) < 1e-5
    xt2, pooled2 = _run_blocks(model, x, b, t, want_fused)
    assert torch.equal(xt, xt2) and torch.equal(pooled, pooled2)


@pytest.mark.parametrize("flag", [True, False], ids=["fused", "round-2"])
@pytest.mark.parametrize("d,heads,img,patch,b,depth,bott",
                         [(384, 6, 32, 16, 53, 2, 32), (192, 3, 224, 16, 2, 1, 64), (384, 6, 32, 16, 3, 1, 80)])
def test_forward_cols_is_the_blocks_on_its_tokens(d, heads, img, patch, b, depth, bott, flag, monkeypatch):
    """forward_cols against a direct call of the block loop on the tokens it assembled: the whole stream and the pooled rows, bit for
    bit (pool = "mean_patches": every patch row reaches the output)."""
    from snuffy_amd import ops, vit
    monkeypatch.setattr(vit, "BF16_FUSED_BLOCK", flag)
    model, _ = _model(d, heads, depth, bott, True, img, patch, "mean_patches")
    p = (img // patch) ** 2
    t = p + 1
    cols = torch.randn(b * p, 3 * patch * patch, generator=torch.Generator().manual_seed(b)).to(BF).to(DEV)
    kept = {}
    real = ops.vit_assemble_tokens

    def keeping(*a, **kw):
        kept["stream"] = real(*a, **kw)
        kept["tokens"] = kept["stream"].clone()
        return kept["stream"]
    monkeypatch.setattr(ops, "vit_assemble_tokens", keeping)
    out = model.forward_cols(cols, b, img, img)
    fused = flag and model._fused_ok()
    assert fused == (flag and bott != 80)
    xt, pooled = _run_blocks(model, kept["tokens"], b, t, fused)
    assert not torch.equal(kept["stream"], kept["tokens"])
    assert torch.equal(xt, kept["stream"]) and torch.equal(pooled, out)


# -- 3. the fold's envelope, kernel level -----------------------------------------------------------------------------------------
FOLD_M = 300
FOLD_R = (0, 1, 4, 8, 16, 64)          # 8 is beyond the issue's set: it brackets the crossing of the flat 1e-2 gate
FOLD_SPECIAL = ("outliers", "scaled_1e3", "scaled_1e-3", "near_constant")


def _fold_rows(case, d):
    """-> (rows [300, d] f32, r): sigma randn + mu with r = mu / sigma (sign alternating by row) for a number; for the special rows r is
    the largest |mean| / sqrt(var + eps) of the rows themselves (fp64)."""
    g = torch.Generator().manual_seed(100 * d + (FOLD_R + FOLD_SPECIAL).index(case))      # never the weights' seed
    sign = (1.0 - 2.0 * (torch.arange(FOLD_M) % 2)).unsqueeze(1)
    z = torch.randn(FOLD_M, d, generator=g)
    if not isinstance(case, str):
        return z + float(case) * sign, float(case)
    if case == "outliers":
        x = z.clone()
        x[:, 5], x[:, 77] = 150.0, -60.0
    elif case == "scaled_1e3":
        x = 1e3 * (z + sign)
    elif case == "scaled_1e-3":
        x = 1e-3 * (z + sign)                       # var = eps
    else:
        x = 1.0 + 1e-5 * z                          # var = 1e-10 << eps: every row rounds to the constant 1 in bf16
    x64 = x.double()
    r = (x64.mean(1).abs() / (x64.var(1, unbiased=False) + VIT_EPS).sqrt()).max()
    return x, float(r)


@pytest.mark.parametrize("case", FOLD_R + FOLD_SPECIAL, ids=lambda c: "r%d" % c if not isinstance(c, str) else c)
@pytest.mark.parametrize("d", [192, 384, 768])
def test_fold_envelope(d, case):
    from snuffy_amd import ops
    n, eps = 3 * d, VIT_EPS
    x, r = _fold_rows(case, d)
    g = torch.Generator().manual_seed(50000 + d)
    gam, bet = 1.0 + 0.2 * torch.randn(d, generator=g), 0.2 * torch.randn(d, generator=g)
    w0, b0 = torch.randn(n, d, generator=g) / d ** 0.5, 0.2 * torch.randn(n, generator=g)
    x64 = x.double()
    mean, var = x64.mean(1), x64.var(1, unbiased=False)
    rstd = (var + eps).rsqrt()
    # mean: atol 1e-5 max(1, |mu|); the special rows have no nominal mu: their own largest |mean| and spread stand in (scale invariance)
    scale = max(1.0, r) if not isinstance(case, str) else max(1.0, float(mean.abs().max()), float(var.max().sqrt()))
    xd = x.to(DEV)
    # statistics from the rows (two passes) ...
    stats, xb = ops.vit_row_stats(xd, eps=eps, want_bf16=True)
    assert torch.equal(xb.cpu(), x.to(BF))
    e_mean = float((stats[:, 0].cpu().double() - mean).abs().max())
    e_rstd = float(((stats[:, 1].cpu().double() - rstd) / rstd).abs().max())
    # ... and from the moment pairs gemm_bf16_resid_ leaves (x += 0 W^T + 0: the stream is unchanged, the pairs are those of x)
    part = torch.full((FOLD_M, d // 32, 2), float("nan"), device=DEV)
    xb2 = torch.empty(FOLD_M, d, dtype=BF, device=DEV)
    x_same = xd.clone()
    ops.gemm_bf16_resid_(x_same, torch.zeros(FOLD_M, 96, dtype=BF, device=DEV), torch.zeros(d, 96, dtype=BF, device=DEV),
                         torch.zeros(d, device=DEV), xb2, part)
    assert torch.equal(x_same, xd) and torch.equal(xb2, xb)
    stats_p, _ = ops.vit_row_stats(part=part, d=d, eps=eps)
    e_mean_p = float((stats_p[:, 0].cpu().double() - mean).abs().max())
    e_rstd_p = float(((stats_p[:, 1].cpu().double() - rstd) / rstd).abs().max())
    bound_p = 16 * (1 + r * r) * 2.0 ** -24
    # the fold
    wf = (w0.double() * gam.double()).float().to(BF)
    cs = wf.double().sum(1).float()
    bfold = (w0.double() @ bet.double() + b0.double()).float()
    out = ops.gemm_bf16_lnfold(xb, wf.to(DEV), cs.to(DEV), bfold.to(DEV), stats).cpu().double()
    ref = F.layer_norm(x64, (d,), gam.double(), bet.double(), eps) @ w0.double().t() + b0.double()
    unfused = F.layer_norm(x, (d,), gam, bet, eps).to(BF).double() @ w0.to(BF).double().t() + b0.double()
    emu = rstd[:, None] * (x.to(BF).double() @ wf.double().t() - mean[:, None] * cs.double()) + bfold.double()
    e_fold, e_u, e_emu = rel_err(out, ref), rel_err(unfused, ref), rel_err(emu, ref)
    own = float((out - emu).abs().max()) / max(1.0, float(emu.abs().max()))
    bound_fold = 1.5 * math.sqrt(1 + r * r) * e_u + 2.0 ** -9
    print("MEASURED vit fold d %3d %-13s r %8.2f  mean %.2e / %.2e (pairs)  rstd %.2e / %.2e (pairs, bound %.2e)  fold %.3e  "
          "unfused recipe e_u %.3e  fold in fp64 %.3e  bound %.3e  ratio to sqrt(1 + r^2) e_u %.2f  to own arithmetic %.2e"
          % (d, case, r, e_mean, e_mean_p, e_rstd, e_rstd_p, bound_p, e_fold, e_u, e_emu, bound_fold,
             e_fold / (math.sqrt(1 + r * r) * e_u), own))
    assert e_mean <= 1e-5 * scale and e_mean_p <= 1e-5 * scale
    assert e_rstd <= 1e-5
    assert e_rstd_p <= bound_p
    assert e_fold <= bound_fold
    assert own <= 4.5e-3                             # the gate of test_gemm_bf16_lnfold_is_layernorm_then_linear, at every r
    # the pairs' statistics feed the same kernel: the fold on them stays inside the same envelope
    out_p = ops.gemm_bf16_lnfold(xb, wf.to(DEV), cs.to(DEV), bfold.to(DEV), stats_p).cpu().double()
    assert rel_err(out_p, ref) <= bound_fold
