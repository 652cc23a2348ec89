"""Every register form of the row passes of csrc/rowops.hip -- the critic, LayerNorm forward / images / backward and the mean-pooled head
(plain, deferred, varlen) -- at both edges of the form, through one, two and three trips of the grid-stride loop, against fp64; and the
column sums at the forms their own dispatch has.  tests/row_forms.py is the table (widths, row counts, gates, operands, references);
test_row_forms_host.py proves it reaches every (entry, form).  Every figure is a max over all elements; each case prints its figures in
lines that start with "row_forms" (profiles/row_forms.txt is their summary)."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import row_forms as RF
from tests.helpers import BF, DEV, _ops

pytestmark = pytest.mark.gpu

ALL = pytest.mark.parametrize("case", RF.CASES, ids=RF.case_id)
LONG = pytest.mark.parametrize("case", RF.LONG_CASES, ids=RF.case_id)
HL = pytest.mark.parametrize("d", RF.WIDTHS_HL)


@pytest.fixture(scope="module")
def per_trip():
    return RF.rows_per_trip()


@pytest.fixture(scope="module")
def head_per_trip():
    return RF.head_rows_per_trip()


def _form(d, aligned):
    """The form of the case; where the operands are placed off their boundary, the scalar form must be the one chosen."""
    form = RF.row_form(d, aligned)
    if not aligned:
        assert form[0] == 1 and RF.row_form(d, True)[0] == 4, (d, form)
    return form


def _report(entry, d, aligned, n, **figures):
    print("row_forms %-22s form %s d %4d%s n %5d  %s" % (entry, "%dx%-2d" % _form(d, aligned), d, "" if aligned else " off4", n,
                                                         "  ".join("%s %.3e" % kv for kv in figures.items())))


def _err(got, ref):
    return (got.double() - ref).abs().max().item()


def _bits(t):
    return t.view(torch.int16)


# ---- LayerNorm forward ---------------------------------------------------------------------------------------------------------------------
def _layernorm(d, aligned, n, per_trip):
    ops = _ops()
    g = RF.gen(1, d, n)
    x = RF.rows_operand(g, n, d, 3.0, 1.0)
    gam, bet = RF.columns(g, d), RF.columns(g, d)
    xa, ga, ba = (RF.place(t, aligned) for t in (x, gam, bet))
    # f32 with the affine and the statistics
    out, mean, rstd = ops.layernorm_rows(xa, ga, ba, RF.EPS, want_stats=True)
    rs = 1.0 / torch.sqrt(x.double().var(1, unbiased=False) + RF.EPS)
    e_out, e_mean = _err(out, RF.ln64(x, gam, bet)), _err(mean, x.double().mean(1))
    e_rstd = _err(rstd, rs) / rs.abs().max().item()
    # bf16 without the affine
    ob = ops.layernorm_rows(xa, None, None, RF.EPS, out_dtype=BF)
    e_bf = _err(ob, RF.ln64(x))
    # patched rows: the first, the last, one inside and the first of the last trip
    slot, rows = RF.slot_of(n, RF.marked_rows(n, per_trip))
    patch = RF.rows_operand(g, rows.numel(), d, 3.0, 1.0)
    pa = RF.place(patch, aligned)
    y = x.clone()
    y[rows] = patch
    outp = ops.layernorm_rows(xa, ga, ba, RF.EPS, slot=slot, patch_rows=pa)
    e_patch = _err(outp, RF.ln64(y, gam, bet))
    keep = torch.ones(n, dtype=torch.bool, device=DEV)
    keep[rows] = False
    assert torch.equal(outp[keep], out[keep])
    # the patched rows re-normalised into existing buffers: bf16 without the affine, f32 with it; the other rows keep their bits
    buf, buf32 = RF.place(ob.clone(), True), RF.place(out.clone(), aligned)
    ops.layernorm_rows(pa, None, None, RF.EPS, out=buf, out_row_idx=rows)
    ops.layernorm_rows(pa, ga, ba, RF.EPS, out=buf32, out_row_idx=rows)
    e_buf, e_buf32 = _err(buf[rows], RF.ln64(patch)), _err(buf32[rows], RF.ln64(patch, gam, bet))
    assert torch.equal(_bits(buf[keep]), _bits(ob[keep])) and torch.equal(buf32[keep], out[keep])
    _report("layernorm_rows", d, aligned, n, out=e_out, mean=e_mean, rstd_rel=e_rstd, bf16=e_bf, patch=e_patch, into_bf16=e_buf,
            into_f32=e_buf32)
    assert e_out < RF.LN_F32 and e_patch < RF.LN_F32 and e_buf32 < RF.LN_F32
    assert e_bf < RF.LN_BF16 and e_buf < RF.LN_BF16
    assert e_mean < RF.LN_MEAN and e_rstd < RF.LN_RSTD_REL


@ALL
def test_layernorm_rows_short(case, per_trip):
    for n in RF.SHORT_ROWS:
        _layernorm(*case, n, per_trip)


@LONG
@pytest.mark.parametrize("which", [0, 1], ids=["two-trips", "three-trips"])
def test_layernorm_rows_long(case, which, per_trip):
    _layernorm(*case, RF.long_rows(per_trip)[which], per_trip)


# ---- the split images ------------------------------------------------------------------------------------------------------------------------
def _images(d, n, per_trip):
    """split3 / hl / hl patch == the split of layernorm_rows' f32 rows, bit for bit."""
    ops = _ops()
    g = RF.gen(2, d, n)
    x = RF.rows_operand(g, n, d, 3.0, 1.0)
    gam, bet = RF.columns(g, d), RF.columns(g, d)
    slot, rows = RF.slot_of(n, RF.marked_rows(n, per_trip))
    patch = RF.rows_operand(g, rows.numel(), d, 3.0, 1.0)
    for kw in ({}, {"slot": slot, "patch_rows": patch}):
        hi, lo = RF.split(ops.layernorm_rows(x, gam, bet, RF.EPS, **kw))
        img3 = ops.layernorm_rows_split3(x, gam, bet, RF.EPS, **kw)
        assert img3.shape == (n, 3 * d) and img3.dtype == BF
        a, b, c = RF.decode_split3(img3, d)
        assert torch.equal(_bits(a), _bits(hi)) and torch.equal(_bits(b), _bits(hi)) and torch.equal(_bits(c), _bits(lo))
        if d % 32 == 0:
            img = ops.layernorm_rows_hl(x, gam, bet, RF.EPS, **kw)
            assert img.shape == (n, 2 * d) and img.dtype == BF
            a, b = RF.decode_hl(img, d)
            assert torch.equal(_bits(a), _bits(hi)) and torch.equal(_bits(b), _bits(lo))
    if d % 32:
        return
    # hl patch: LayerNorm(x + addend) of a few rows over those rows of an existing image, the others untouched ...
    img = ops.layernorm_rows_hl(x, None, None, RF.EPS)
    before = img.clone()
    add = RF.rows_operand(g, rows.numel(), d, 1.0, 0.0)
    keep = torch.ones(n, dtype=torch.bool, device=DEV)
    keep[rows] = False
    for kw in ({}, {"gamma": gam, "beta": bet}):
        img.copy_(before)
        ops.layernorm_rows_hl_patch_(img, rows, patch, add, eps=RF.EPS, **kw)
        hi, lo = RF.split(ops.layernorm_rows(patch + add, kw.get("gamma"), kw.get("beta"), RF.EPS))
        a, b = RF.decode_hl(img[rows], d)
        assert torch.equal(_bits(a), _bits(hi)) and torch.equal(_bits(b), _bits(lo))
        assert torch.equal(_bits(img[keep]), _bits(before[keep]))
    # ... and of every row, to a permutation of the rows (the patch kernel's own loop runs as often as the plain one's)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(n + d)).to(DEV)
    img = torch.zeros(n, 2 * d, dtype=BF, device=DEV)
    ops.layernorm_rows_hl_patch_(img, perm, x, None, gamma=gam, beta=bet, eps=RF.EPS)
    hi, lo = RF.split(ops.layernorm_rows(x, gam, bet, RF.EPS))
    a, b = RF.decode_hl(img[perm], d)
    assert torch.equal(_bits(a), _bits(hi)) and torch.equal(_bits(b), _bits(lo))


@pytest.mark.parametrize("d", RF.WIDTHS_HL + RF.WIDTHS_VEC1)
def test_images_short(d, per_trip):
    for n in RF.SHORT_ROWS:
        _images(d, n, per_trip)


@pytest.mark.parametrize("d", RF.LONG_HL + [193, 1025])
@pytest.mark.parametrize("which", [0, 1], ids=["two-trips", "three-trips"])
def test_images_long(d, which, per_trip):
    _images(d, RF.long_rows(per_trip)[which], per_trip)


# ---- LayerNorm backward ----------------------------------------------------------------------------------------------------------------------
def _backward(d, aligned, n):
    ops = _ops()
    g = RF.gen(3, d, n)
    x = RF.rows_operand(g, n, d, 2.0, 0.5)
    gamma = RF.columns(g, d, scale=0.3, shift=1.0)
    dy = RF.columns(g, n, d)
    res = RF.columns(g, n, d)
    lead = 4                                                            # the strided view: columns 4 .. 4 + d of a wider buffer whose
    wide = RF.columns(g, n, lead + (d + 3) // 4 * 4 + 4)                # pitch is a multiple of 4 floats, so the kernel takes it in place
    dys = wide[:, lead:lead + d]
    assert dys.stride(0) > d and dys.data_ptr() % 16 == 0
    xa, ga, dya, resa, row_a = (RF.place(t, aligned) for t in (x, gamma, dy, res, dy[0].contiguous()))
    cases = [("f32", dya, dy, None, None), ("residual", dya, dy, resa, res), ("bf16", dy.to(BF), dy.to(BF), None, None),
             ("strided", dys, dys, None, None), ("broadcast", row_a, dy[0], resa, res)]
    figures, first = {}, None
    for name, dyv, dy_ref, resv, res_ref in cases:
        dx, dxb, dgam, dbet = ops.layernorm_rows_bwd(xa, dyv, ga, RF.EPS, residual=resv, want_dx_bf16=True)
        rdx, rg, rb = RF.ln_bwd64(x, dy_ref, gamma, res_ref)
        scale = rdx.abs().max().item()
        e_dx, e_g, e_b = _err(dx, rdx), _err(dgam, rg), _err(dbet, rb)
        figures[name + "_dx_rel"] = e_dx / scale if scale else e_dx
        figures[name + "_dgamma"], figures[name + "_dbeta"] = e_g, e_b
        assert e_dx <= RF.BWD_DX_REL * scale + RF.REF64_FLOOR, (name, e_dx, scale)
        assert torch.equal(_bits(dxb), _bits(dx.to(BF))), name
        # every column against the bound (a max over the columns, never their mean)
        assert e_g <= RF.BWD_PARAM_REL * max(1.0, rg.abs().max().item()), (name, e_g)
        assert e_b <= RF.BWD_PARAM_REL * max(1.0, rb.abs().max().item()), (name, e_b)
        if first is None:
            first = (dx, dgam, dbet)
    _report("layernorm_rows_bwd", d, aligned, n, **figures)
    # no gamma, no partial sums
    dx, dxb, a, b = ops.layernorm_rows_bwd(xa, dya, None, RF.EPS, want_param_grads=False)
    rdx, _, _ = RF.ln_bwd64(x, dy, None, None)
    assert a is None and b is None and dxb is None and _err(dx, rdx) <= RF.BWD_DX_REL * rdx.abs().max().item() + RF.REF64_FLOOR
    # bf16 dx alone: the rounding of the f32 dx, the same sums
    dx, dxb, dgam, dbet = ops.layernorm_rows_bwd(xa, dya, ga, RF.EPS, want_dx=False, want_dx_bf16=True)
    assert dx is None and torch.equal(_bits(dxb), _bits(first[0].to(BF)))
    assert torch.equal(dgam, first[1]) and torch.equal(dbet, first[2])


@ALL
def test_layernorm_rows_bwd_short(case):
    for n in RF.SHORT_ROWS:
        _backward(*case, n)


@LONG
@pytest.mark.parametrize("which", [0, 1], ids=["two-trips", "three-trips"])
def test_layernorm_rows_bwd_long(case, which, per_trip):
    """The first check of dgamma / dbeta accumulated across trips of the loop."""
    _backward(*case, RF.long_rows(per_trip)[which])


# ---- critic ------------------------------------------------------------------------------------------------------------------------------------
def _critic(d, aligned, n):
    ops = _ops()
    g = RF.gen(4, d, n)
    x = RF.rows_operand(g, n, d, 1.0, 0.0)
    xa = RF.place(x, aligned)
    xhat_ref = ops.layernorm_rows(xa, None, None, RF.EPS, out_dtype=BF)
    for c in (1, 3):
        w, b = RF.columns(g, c, d, scale=1.0 / math.sqrt(d)), RF.columns(g, c)
        wa, bb = RF.place(w, aligned), RF.place(b, aligned)
        s, mv, mi = ops.critic(xa, wa, bb, want_max=True)
        e = _err(s, F.linear(x.double(), w.double(), b.double()))
        _report("critic", d, aligned, n, **{"scores_c%d" % c: e})
        assert s.shape == (n, c) and e < RF.CRITIC
        mvr, mir = s.cpu().max(dim=0)
        assert torch.equal(mv.cpu(), mvr) and torch.equal(mi.cpu(), mir)
        s2, xhat = ops.critic_ln(xa, wa, bb, RF.EPS)
        assert torch.equal(s2, s) and torch.equal(_bits(xhat), _bits(xhat_ref))


@ALL
def test_critic_short(case):
    for n in RF.SHORT_ROWS:
        _critic(*case, n)


@LONG
@pytest.mark.parametrize("which", [0, 1], ids=["two-trips", "three-trips"])
def test_critic_long(case, which, per_trip):
    _critic(*case, RF.long_rows(per_trip)[which])


def _critic_ln_hl(d, n):
    ops = _ops()
    g = RF.gen(5, d, n)
    x = RF.rows_operand(g, n, d, 2.0, 0.3)
    gam, bet = RF.columns(g, d, scale=0.1, shift=1.0), RF.columns(g, d, scale=0.1)
    for c in (1, 3):
        w, b = RF.columns(g, c, d, scale=1.0 / math.sqrt(d)), RF.columns(g, c)
        s_ref = ops.critic(x, w, b)
        for ga, be in ((gam, bet), (None, None)):
            s, img = ops.critic_ln_hl(x, w, b, ga, be, RF.EPS)
            assert torch.equal(s, s_ref)
            assert torch.equal(_bits(img), _bits(ops.layernorm_rows_hl(x, ga, be, RF.EPS))), (d, n, c, ga is None)


@HL
def test_critic_ln_hl_short(d):
    for n in RF.SHORT_ROWS:
        _critic_ln_hl(d, n)


@pytest.mark.parametrize("d", RF.LONG_HL)
@pytest.mark.parametrize("which", [0, 1], ids=["two-trips", "three-trips"])
def test_critic_ln_hl_long(d, which, per_trip):
    _critic_ln_hl(d, RF.long_rows(per_trip)[which])


@LONG
def test_critic_select_three_trips(case, per_trip):
    """The critic pass that counts the selector's histogram, with and without the normalised copy: the plain critic's scores bit for bit,
    and the selection that starts from the histogram is the top-k of those scores."""
    ops = _ops()
    d, aligned = case
    n = max(2 * per_trip + 5, ops.SELECT_FUSED_MIN_N)                   # the fused form starts at 16385 rows
    assert RF.trips(n, per_trip) >= 3
    g = RF.gen(6, d, n)
    x = RF.rows_operand(g, n, d, 1.0, 0.0)
    w, b = RF.columns(g, 1, d, scale=1.0 / math.sqrt(d)), RF.columns(g, 1)
    s_ref = ops.critic(x, w, b)
    e = _err(s_ref, F.linear(x.double(), w.double(), b.double()))
    _report("critic_select", d, aligned, n, scores=e)
    assert e < RF.CRITIC
    want = torch.sort(s_ref.view(-1), descending=True, stable=True)[1][:200]
    for eps in (None, RF.EPS):
        got = ops.critic_select(x, w, b, eps)
        assert got is not None
        s, xhat = got
        assert torch.equal(s, s_ref)
        if eps is None:
            assert xhat is None
        else:
            assert torch.equal(_bits(xhat), _bits(ops.layernorm_rows(x, None, None, eps, out_dtype=BF)))
        assert torch.equal(ops.topk(s.view(-1), 200), want)


# ---- the mean-pooled head ----------------------------------------------------------------------------------------------------------------------
def _head_operands(g, n, d, c, marked):
    z = RF.rows_operand(g, n, d, 2.0, 0.5)
    gam, bet = RF.columns(g, d), RF.columns(g, d)
    w, b = RF.columns(g, c, d, scale=1.0 / math.sqrt(d)), RF.columns(g, c)
    slot, rows = RF.slot_of(n, marked)
    delta = RF.columns(g, rows.numel(), d)
    addb = RF.columns(g, n, d).to(BF)
    bias = RF.columns(g, d)
    zz = z.double() + addb.double() + bias.double()
    zz[rows] += delta.double()
    return z, gam, bet, w, b, slot, delta, addb, bias, zz


def _head(d, aligned, n, head_per_trip):
    ops = _ops()
    for c in (1, 3):
        g = RF.gen(7, d, n, c)
        z, gam, bet, w, b, slot, delta, addb, bias, zz = _head_operands(g, n, d, c, RF.marked_rows(n, head_per_trip))
        za, ga, ba, wa, bb, da, bia = (RF.place(t, aligned) for t in (z, gam, bet, w, b, delta, bias))
        logits, pooled, zo = ops.ln_mean_head(za, ga, ba, RF.EPS, wa, bb)
        p_ref, l_ref = RF.head64(z.double(), gam, bet, w, b)
        e_p, e_l = _err(pooled, p_ref), _err(logits, l_ref)
        assert zo is None and logits.shape == (c,)
        l2, p2, zo = ops.ln_mean_head(za, ga, ba, RF.EPS, wa, bb, add_bf16=addb, add_bias=bia, slot=slot, delta_rows=da, want_z=True)
        p_ref, l_ref = RF.head64(zz, gam, bet, w, b)
        e_p2, e_l2, e_z = _err(p2, p_ref), _err(l2, l_ref), _err(zo, zz)
        _report("ln_mean_head", d, aligned, n, **{"pooled_c%d" % c: e_p, "logits": e_l, "pooled_addends": e_p2, "logits_addends": e_l2,
                                                  "z_out": e_z})
        assert max(e_p, e_l, e_p2, e_l2, e_z) < RF.HEAD


@ALL
def test_ln_mean_head_short(case, head_per_trip):
    for n in RF.SHORT_ROWS:
        _head(*case, n, head_per_trip)


@LONG
@pytest.mark.parametrize("which", [0, 1], ids=["two-trips", "three-trips"])
def test_ln_mean_head_long(case, which, head_per_trip):
    _head(*case, RF.long_rows(head_per_trip)[which], head_per_trip)


@pytest.mark.parametrize("d", RF.DEFERRED_WIDTHS)
@pytest.mark.parametrize("addends", ["none", "all"])
def test_deferred_head_three_trips(d, addends, head_per_trip):
    """The head that adds the unsummed K part as it reads, over a tile map that differs in every row band, column block and trip: bit for
    bit the plain head on the summed rows, and both within the head's bound of fp64 (so the pair cannot be wrong together)."""
    ops = _ops()
    n, c = 2 * head_per_trip + 261, 2
    g = RF.gen(8, d, n)
    z, gam, bet, w, b, slot, delta, addb, bias, zz = _head_operands(g, n, d, c, RF.marked_rows(n, head_per_trip))
    dk = RF.synthetic_deferred(g, n, d, head_per_trip)
    assert int((dk.tile_map != 0).sum()) == dk.slabs.shape[0] >= 3 * ((d + 255) // 256)
    zsum = dk.add_to(z)
    kw = dict(add_bf16=addb, add_bias=bias, slot=slot, delta_rows=delta) if addends == "all" else {}
    z64 = zsum.double() + (zz - z.double() if addends == "all" else 0)
    p_ref, l_ref = RF.head64(z64, gam, bet, w, b)
    for want_z in (False, True):
        got = ops.ln_mean_head(z, gam, bet, RF.EPS, w, b, want_z=want_z, deferred=dk, **kw)
        ref = ops.ln_mean_head(zsum, gam, bet, RF.EPS, w, b, want_z=want_z, **kw)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
        e_l, e_p = _err(got[0], l_ref), _err(got[1], p_ref)
        e_z = 0.0
        if want_z:
            assert torch.equal(got[2], ref[2])
            e_z = _err(got[2], z64)
        else:
            assert got[2] is None
        _report("ln_mean_head deferred", d, True, n, logits=e_l, pooled=e_p, z_out=e_z)
        assert max(e_l, e_p, e_z) < RF.HEAD


@pytest.mark.parametrize("d", RF.VARLEN_WIDTHS)
@pytest.mark.parametrize("addends", ["none", "all"])
def test_varlen_head(d, addends, head_per_trip):
    """Every bag of a packed batch (one, two and three trips among them): its own ln_mean_head call bit for bit, and fp64."""
    ops = _ops()
    r, c = head_per_trip, 2
    sizes = [1, 3, r + 5, 37, 2 * r + 9]
    packed = ops.PackedBags(sizes, DEV)
    total, off = packed.total, [int(o) for o in packed.host]
    marked = sorted({o for o in off[:-1]} | {o - 1 for o in off[1:]} | {off[4] + 2 * r, off[2] + r + 4})
    g = RF.gen(9, d)
    z, gam, bet, w, b, slot, delta, addb, bias, zz = _head_operands(g, total, d, c, marked)
    kw = dict(add_bf16=addb, add_bias=bias, slot=slot, delta_rows=delta) if addends == "all" else {}
    z64 = zz if addends == "all" else z.double()
    logits, pooled = ops.ln_mean_head_varlen(z, packed, gam, bet, RF.EPS, w, b, **kw)
    assert logits.shape == (len(sizes), c) and pooled.shape == (len(sizes), d)
    for i, n in enumerate(sizes):
        o = off[i]
        own_kw = dict(kw)
        if kw:
            own_kw.update(add_bf16=addb[o:o + n], slot=slot[o:o + n])
        l_own, p_own, _ = ops.ln_mean_head(z[o:o + n], gam, bet, RF.EPS, w, b, **own_kw)
        assert torch.equal(logits[i], l_own) and torch.equal(pooled[i], p_own), (i, n)
        p_ref, l_ref = RF.head64(z64[o:o + n], gam, bet, w, b)
        e_l, e_p = _err(logits[i], l_ref), _err(pooled[i], p_ref)
        _report("ln_mean_head varlen", d, True, n, logits=e_l, pooled=e_p)
        assert max(e_l, e_p) < RF.HEAD


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_too_wide_is_refused_by_every_entry():
    from snuffy_amd._ffi import SnuffyHipError
    ops = _ops()
    n = 3

    def refused(call, what="too wide"):
        with pytest.raises(SnuffyHipError, match=what):
            call()

    for d, _ in RF.TOO_WIDE + [(RF.TOO_WIDE_HL, True)]:
        assert RF.row_form(d, True) is None
        x, v = torch.zeros(n, d, device=DEV), torch.zeros(d, device=DEV)
        w, b = torch.zeros(1, d, device=DEV), torch.zeros(1, device=DEV)
        slot = torch.full((n,), -1, dtype=torch.int32, device=DEV)
        refused(lambda: ops.critic(x, w, b))
        refused(lambda: ops.critic_ln(x, w, b, RF.EPS))
        refused(lambda: ops.layernorm_rows(x, v, v, RF.EPS))
        refused(lambda: ops.layernorm_rows(x, v, v, RF.EPS, slot=slot, patch_rows=x, out_dtype=BF))
        refused(lambda: ops.layernorm_rows_split3(x, v, v, RF.EPS))
        refused(lambda: ops.layernorm_rows_bwd(x, x, v, RF.EPS))
        refused(lambda: ops.layernorm_rows_bwd(x, v, None, RF.EPS, want_param_grads=False))
        refused(lambda: ops.ln_mean_head(x, v, v, RF.EPS, w, b))
        refused(lambda: ops.ln_mean_head_varlen(x, ops.PackedBags([1, 2], DEV), v, v, RF.EPS, w, b))
        tile_map = torch.zeros(1, (d + 255) // 256, dtype=torch.int32, device=DEV)
        refused(lambda: ops.ln_mean_head(x, v, v, RF.EPS, w, b, deferred=ops.DeferredK(torch.zeros(1, 256, 256, device=DEV), tile_map, None)))
        big = torch.zeros(ops.SELECT_FUSED_MIN_N, d, device=DEV)
        for eps in (None, RF.EPS):
            refused(lambda: ops.critic_select(big, w, b, eps))
        if d % 32 == 0:                                                  # the hl entries take no other width
            refused(lambda: ops.critic_ln_hl(x, w, b, v, v, RF.EPS))
            refused(lambda: ops.layernorm_rows_hl(x, v, v, RF.EPS))
            img = torch.zeros(n, 2 * d, dtype=BF, device=DEV)
            refused(lambda: ops.layernorm_rows_hl_patch_(img, torch.arange(n, device=DEV), x))
        else:
            with pytest.raises((SnuffyHipError, ValueError)):
                ops.critic_ln_hl(x, w, b, v, v, RF.EPS)
            refused(lambda: ops.layernorm_rows_hl(x, v, v, RF.EPS), "multiple of 32")
    torch.cuda.synchronize()


# ---- column sums -----------------------------------------------------------------------------------------------------------------------------------
COLSUM_WIDTHS = [8, 2048, 2056, 4096, 4104, 8192]                       # one, two and four 2048-column chunks a thread, at both edges
DROP = (0.1, 987654321, 5)


def _colsum(n, d):
    ops = _ops()
    g = RF.gen(10, d, n)
    x = RF.rows_operand(g, n, d, 1.0, 0.0)
    w2 = RF.columns(g, n, 2)
    gate = RF.columns(g, n, d).to(BF)
    gate[0, :8] = 0.0                                                   # a zero gate closes
    figures = {}

    def close(name, s, ref):
        figures[name] = _err(s, ref)
        assert figures[name] <= RF.colsum_tol(ref, n), (name, figures[name], RF.colsum_tol(ref, n))

    s, c = ops.colsum_fused(x)
    assert c is None
    close("f32", s, x.double().sum(0))
    s, c = ops.colsum_fused(x, want_bf16=True)
    assert torch.equal(_bits(c), _bits(x.to(BF)))
    close("want_bf16", s, c.double().sum(0))
    s, _ = ops.colsum_fused(x, row_weight=w2[:, 1])                     # the weight as a stride-2 column
    close("weighted", s, (x.double() * w2[:, 1:2].double()).sum(0))
    xb = x.to(BF)
    s, c = ops.colsum_fused(xb)
    assert c is None
    close("bf16", s, xb.double().sum(0))
    want = torch.ops.aten.threshold_backward(xb, gate, 0)
    s, c = ops.colsum_fused(xb.clone(), gate=gate, want_bf16=True)
    assert torch.equal(_bits(c), _bits(want))
    close("gated", s, want.double().sum(0))
    y = xb.clone()
    s2, c2 = ops.colsum_fused(y, gate=gate, inplace=True)
    assert c2 is y and torch.equal(_bits(y), _bits(want)) and torch.equal(s2, s)
    mask = ops.dropout_mask(1, n, d, *DROP, DEV)[0]
    for name, src in (("dropout_f32", x), ("dropout_bf16", xb)):
        want = (src.float() * mask).to(BF)
        s, c = ops.colsum_fused(src, want_bf16=True, dropout=DROP)
        assert torch.equal(_bits(c), _bits(want))
        close(name, s, want.double().sum(0))
    print("row_forms %-22s nch %d d %4d n %5d  %s" % ("colsum_fused", {1: 1, 2: 2}.get((d + 2047) // 2048, 4), d, n,
                                                      "  ".join("%s %.3e" % kv for kv in figures.items())))


@pytest.mark.parametrize("d", COLSUM_WIDTHS)
def test_colsum_fused_short(d):
    for n in (1, 33):
        _colsum(n, d)


@pytest.mark.parametrize("d", COLSUM_WIDTHS)
def test_colsum_fused_long(d):
    n = RF.colsum_long_rows()
    blocks = RF.lib().snf_colsum_blocks(n)
    assert -(-n // blocks) > 32 and n % -(-n // blocks)                  # more than 32 rows a workgroup, the last one ragged
    _colsum(n, d)
