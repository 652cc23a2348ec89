"""The two split-image formats (ops.IMAGE_FORMATS), the parts that need no GPU: what the table holds, the weight image and its decode,
the one cache of weight images and its drop list, and which wrapper each record method calls."""
import pytest
import torch

from snuffy_amd import _ffi, functional as SF, ops, ssl_pretrain as S

FORMATS = sorted(ops.IMAGE_FORMATS)


def decode_restated(name, img):
    """hi + lo of an image, written out from the layouts: hl = [hi(32) | lo(32)] per 32 columns; cat = three planes of which the last
    two are (hi, lo) for rows and (Wl, Wh) for weights."""
    m = img.shape[0]
    if name == "hl":
        k = img.shape[1] // 2
        out = torch.empty(m, k)
        for g in range(k // 32):
            out[:, 32 * g:32 * g + 32] = img[:, 64 * g:64 * g + 32].float() + img[:, 64 * g + 32:64 * g + 64].float()
        return out
    k = img.shape[1] // 3
    return img[:, k:2 * k].float() + img[:, 2 * k:3 * k].float()


def test_the_table_has_the_two_formats_and_the_abi_constants():
    assert FORMATS == ["cat", "hl"] and ops.IMAGE_FORMATS["hl"] is ops.HL and ops.IMAGE_FORMATS["cat"] is ops.CAT
    assert (ops.HL.name, ops.HL.code, ops.HL.granule, ops.HL.width) == ("hl", _ffi.DT_BF16_HL, 32, 2)
    assert (ops.CAT.name, ops.CAT.code, ops.CAT.granule, ops.CAT.width) == ("cat", _ffi.DT_BF16_SPLIT3, 8, 3)
    assert _ffi.DT_BF16_HL != _ffi.DT_BF16_SPLIT3


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("name", FORMATS)
def test_a_weight_decodes_through_the_record(name, transposed):
    """bf16 keeps 8 significant bits, so hi + lo keeps 16 and what is left is below 2^-17 |w| per element (the bound of
    test_vit_trunk_train_host.py)."""
    fmt = ops.IMAGE_FORMATS[name]
    torch.manual_seed(0)
    w = torch.nn.Parameter(torch.randn(160, 96) * torch.logspace(-6, 3, 160).unsqueeze(1))
    want = w.detach().t() if transposed else w.detach()
    img = SF.weight_image(w, fmt, transposed)
    assert img.dtype == torch.bfloat16 and tuple(img.shape) == (want.shape[0], fmt.width * want.shape[1])
    assert SF.weight_image(w, name, transposed) is img                          # the name finds the same entry
    dec = fmt.decode(img)
    assert dec.dtype == torch.float32 and bool(((dec - want).abs() <= 2.0 ** -17 * want.abs()).all())


@pytest.mark.parametrize("name", FORMATS)
def test_decode_and_hi_are_the_layout_restated(name):
    fmt = ops.IMAGE_FORMATS[name]
    g = torch.Generator().manual_seed(1)
    img = (torch.randn(7, fmt.width * 96, generator=g) * torch.logspace(-3, 3, 7).unsqueeze(1)).to(torch.bfloat16)
    assert torch.equal(fmt.decode(img), decode_restated(name, img))
    hi = fmt.hi(img)
    want = torch.cat([img[:, 64 * j:64 * j + 32] for j in range(3)], dim=1) if name == "hl" else img[:, 96:192]
    assert hi.dtype == torch.bfloat16 and torch.equal(hi, want)


def test_invalidate_rebuilds_every_cached_image():
    """An edit through .data moves neither data_ptr nor _version: drop_param_caches is what forgets the images, all four of them."""
    lin = torch.nn.Linear(96, 160)
    cases = [(name, t) for name in FORMATS for t in (False, True)]
    before = {c: SF.weight_image(lin.weight, *c) for c in cases}
    assert all(SF.weight_image(lin.weight, *c) is before[c] for c in cases)
    assert S._image_of_t(lin.weight, "hl") is before[("hl", True)]          # the names the callers had for it
    assert SF.split3_cached(lin.weight, transposed=True) is before[("cat", True)]
    lin.weight.data.add_(1.0)
    assert all(SF.weight_image(lin.weight, *c) is before[c] for c in cases)      # the stale hit this test is about
    SF.drop_param_caches(lin)
    for c in cases:
        img = SF.weight_image(lin.weight, *c)
        want = lin.weight.detach().t() if c[1] else lin.weight.detach()
        assert img is not before[c], c
        assert bool(((ops.IMAGE_FORMATS[c[0]].decode(img) - want).abs() <= 2.0 ** -17 * want.abs()).all()), c


def test_every_attribute_the_cache_sets_is_dropped():
    w = torch.nn.Parameter(torch.randn(64, 32))
    plain = set(vars(w))
    for name in FORMATS:
        for t in (False, True):
            SF.weight_image(w, name, t)
    made = set(vars(w)) - plain
    assert len(made) == 4 and made == set(SF._PARAM_CACHES)


class Recorder:
    """Replaces the named ops wrappers; each call is kept as (name, args, kwargs) and answers a token."""

    def __init__(self, monkeypatch, names):
        self.calls = []
        for name in names:
            assert callable(getattr(ops, name))
            monkeypatch.setattr(ops, name, lambda *a, _n=name, **kw: (self.calls.append((_n, a, kw)), (_n, len(self.calls)))[1])

    def last(self):
        return self.calls[-1]


WRAPPERS = ("split_hl_rows", "split3_rows", "split_hl_weight", "split3_weight", "layernorm_rows_hl", "layernorm_rows_split3", "gemm_hl",
            "gemm_x3", "split_hl_colsum", "split3_colsum", "gemm_tn")


def test_each_method_calls_the_wrapper_it_names(monkeypatch):
    rec = Recorder(monkeypatch, WRAPPERS)
    x, w, g, b, bias, resid = (object() for _ in range(6))
    # rows, LayerNorm
    assert ops.HL.rows(x) == ("split_hl_rows", 1) and rec.last() == ("split_hl_rows", (x,), {})
    assert ops.CAT.rows(x)[0] == "split3_rows" and rec.last() == ("split3_rows", (x,), {})
    ops.HL.layernorm(x, g, b, 1e-6, slot=w, patch_rows=resid)
    assert rec.last() == ("layernorm_rows_hl", (x, g, b, 1e-6), dict(slot=w, patch_rows=resid))
    ops.CAT.layernorm(x, g, b, 1e-6)
    assert rec.last() == ("layernorm_rows_split3", (x, g, b, 1e-6), dict(slot=None, patch_rows=None))
    # weights: the cat kernel applies the column scale itself
    ops.CAT.weight(w, g)
    assert rec.last() == ("split3_weight", (w, g), {})
    wt = torch.arange(64.0).view(2, 32)
    ops.HL.weight(wt)
    assert rec.last()[0] == "split_hl_weight" and rec.last()[1][0] is wt
    ops.HL.weight(wt, torch.full((32,), 2.0))
    assert rec.last()[0] == "split_hl_weight" and torch.equal(rec.last()[1][0], 2.0 * wt)
    # GEMM to fp32, to the own image, to the other format's
    ops.HL.gemm(x, w, bias, "relu", resid=resid)
    assert rec.last() == ("gemm_hl", (x, w, bias, "relu"), dict(hl_out=False, resid=resid))
    ops.HL.gemm(x, w, bias, image=ops.HL)
    assert rec.last() == ("gemm_hl", (x, w, bias, "none"), dict(hl_out=True, resid=None))
    ops.CAT.gemm(x, w, bias, "relu", resid=resid)
    assert rec.last() == ("gemm_x3", (x, w, bias, "relu"), dict(split3=False, hl_out=False, resid=resid))
    ops.CAT.gemm(x, w, image=ops.CAT)
    assert rec.last() == ("gemm_x3", (x, w, None, "none"), dict(split3=True, hl_out=False, resid=None))
    ops.CAT.gemm(x, w, image=ops.HL)
    assert rec.last() == ("gemm_x3", (x, w, None, "none"), dict(split3=False, hl_out=True, resid=None))
    n = len(rec.calls)
    with pytest.raises(ValueError, match="gemm_hl"):
        ops.HL.gemm(x, w, image=ops.CAT)                                       # the one-pass kernel writes no cat image
    # split + column sums: hl is gated by the activation's image, cat by its hi plane; dropout exists on the hl side only
    act = torch.zeros(3, 3 * 16, dtype=torch.bfloat16)
    ops.HL.colsum(x, gate=act, out=w, col=32, want_colsum=False, dropout=(0.1, 2, 3))
    assert rec.last() == ("split_hl_colsum", (x,), dict(gate_hl=act, out=w, col=32, want_colsum=False, dropout=(0.1, 2, 3)))
    ops.CAT.colsum(x, gate=act, out=w, col=8)
    name, args, kw = rec.last()
    assert (name, args) == ("split3_colsum", (x,)) and kw["out"] is w and kw["col"] == 8 and kw["want_colsum"] is True
    assert tuple(kw["gate"].shape) == (3, 16) and kw["gate"].data_ptr() == act[:, 16:].data_ptr()
    ops.CAT.colsum(x)
    assert rec.last()[2]["gate"] is None
    with pytest.raises(ValueError, match="split3_colsum"):
        ops.CAT.colsum(x, dropout=(0.1, 2, 3))
    assert len(rec.calls) == n + 3
    # the bag-axis contraction
    ops.HL.tn(x, w, 64, 96)
    assert rec.last() == ("gemm_tn", (x, w, 64, 96), dict(hl=True))
    ops.CAT.tn(x, w, 64, 96)
    assert rec.last() == ("gemm_tn", (x, w, 64, 96, (64, 128), (96, 192)), {})
