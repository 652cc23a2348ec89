"""The two split-image formats (ops.IMAGE_FORMATS) on the device: every record method is the launch of the wrapper it names -- the same
bits -- at the smallest shapes with one row, a row count off every tile and more than one block, one and three column granules; and
rows -> decode returns the matrix to the precision the format keeps."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
FORMATS = ("hl", "cat")
ROWS = (1, 33, 257)


def _x(m, k, seed):
    """[m, k] f32, both signs, magnitudes from 1e-3 (first column) to 1e3 (last)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(m, k, generator=g).clamp(-1, 1) * torch.logspace(-3, 3, k).unsqueeze(0)).to(DEV)


def _wrappers(name):
    from snuffy_amd import ops
    if name == "hl":
        return ops.HL, ops.split_hl_rows, ops.layernorm_rows_hl, ops.split_hl_colsum, "gate_hl"
    return ops.CAT, ops.split3_rows, ops.layernorm_rows_split3, ops.split3_colsum, "gate"


@pytest.mark.parametrize("m", ROWS)
@pytest.mark.parametrize("name", FORMATS)
def test_rows_layernorm_and_colsum_are_the_wrappers_launches(name, m):
    fmt, rows, layernorm, colsum, gate_kw = _wrappers(name)
    for k in (fmt.granule, 3 * fmt.granule):
        x = _x(m, k, 10 * m + k)
        img = fmt.rows(x)
        assert tuple(img.shape) == (m, fmt.width * k) and torch.equal(img, rows(x))
        dec = fmt.decode(img)
        assert bool(((dec - x).abs() <= 2.0 ** -17 * x.abs()).all())            # hi + lo keeps 16 significant bits
        gamma, beta = torch.linspace(0.5, 2.0, k, device=DEV), torch.linspace(-1.0, 1.0, k, device=DEV)
        assert torch.equal(fmt.layernorm(x, gamma, beta, 1e-6), layernorm(x, gamma, beta, 1e-6))
        if m > 1:                                                               # rows 0 and m - 1 read from patch_rows
            slot = torch.full((m,), -1, dtype=torch.int32, device=DEV)
            slot[0], slot[m - 1] = 1, 0
            patch = _x(2, k, 77)
            assert torch.equal(fmt.layernorm(x, None, None, 1e-5, slot=slot, patch_rows=patch),
                               layernorm(x, None, None, 1e-5, slot=slot, patch_rows=patch))
        # split + column sums: plain, gated by an activation's image, into a wider image one granule in
        act = fmt.rows(_x(m, k, 5).relu())
        gate = act if name == "hl" else act[:, k:2 * k]
        for got, want in ((fmt.colsum(x), colsum(x)), (fmt.colsum(x, gate=act), colsum(x, **{gate_kw: gate}))):
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        wide = [torch.zeros(m, fmt.width * (fmt.granule + k), dtype=torch.bfloat16, device=DEV) for _ in range(2)]
        got = fmt.colsum(x, out=wide[0], col=fmt.granule, want_colsum=False)
        want = colsum(x, out=wide[1], col=fmt.granule, want_colsum=False)
        assert got[0] is wide[0] and got[1] is None and want[1] is None and torch.equal(wide[0], wide[1])
        assert torch.equal(fmt.decode(wide[0])[:, fmt.granule:], dec) and not bool(fmt.decode(wide[0])[:, :fmt.granule].any())


@pytest.mark.parametrize("m", ROWS)
def test_hl_colsum_dropout_is_the_wrappers_launch(m):
    from snuffy_amd import ops
    x = _x(m, 96, m)
    got, want = ops.HL.colsum(x, dropout=(0.25, 11, 3)), ops.split_hl_colsum(x, dropout=(0.25, 11, 3))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("m", ROWS)
@pytest.mark.parametrize("name", FORMATS)
def test_gemms_are_the_wrappers_launches(name, m):
    from snuffy_amd import ops
    fmt = ops.IMAGE_FORMATS[name]
    for k in (32, 96):
        a = fmt.rows(_x(m, k, m + k))
        for n in (8, 40, 32, 96):
            g = torch.Generator().manual_seed(n)
            w = fmt.weight((torch.randn(n, k, generator=g) * torch.logspace(-3, 3, n).unsqueeze(1)).to(DEV))
            bias = torch.randn(n, generator=g).to(DEV)
            if n in (8, 40):                                                    # fp32 results: plain, with an activation, with a residual
                resid = _x(m, n, 3)
                if name == "hl":
                    want = (ops.gemm_hl(a, w), ops.gemm_hl(a, w, bias, "relu"), ops.gemm_hl(a, w, bias, resid=resid))
                else:
                    want = (ops.gemm_x3(a, w), ops.gemm_x3(a, w, bias, "relu"), ops.gemm_x3(a, w, bias, resid=resid))
                got = (fmt.gemm(a, w), fmt.gemm(a, w, bias, "relu"), fmt.gemm(a, w, bias, resid=resid))
                assert all(y.dtype == torch.float32 and tuple(y.shape) == (m, n) for y in got)
            else:                                                               # image results: the format's own; cat also writes hl
                if name == "hl":
                    want = (ops.gemm_hl(a, w, bias, "relu", hl_out=True),)
                    got = (fmt.gemm(a, w, bias, "relu", image=fmt),)
                else:
                    want = (ops.gemm_x3(a, w, bias, "relu", split3=True), ops.gemm_x3(a, w, bias, hl_out=True))
                    got = (fmt.gemm(a, w, bias, "relu", image=fmt), fmt.gemm(a, w, bias, image=ops.HL))
                    assert tuple(got[1].shape) == (m, 2 * n)
                assert tuple(got[0].shape) == (m, fmt.width * n)
            assert all(torch.equal(y, z) for y, z in zip(got, want)), (k, n)


@pytest.mark.parametrize("name", FORMATS)
def test_the_contraction_is_gemm_tn(name):
    """1025 rows: one past gemm_tn's minimum, so the last 32-row step is cut short."""
    from snuffy_amd import ops
    fmt = ops.IMAGE_FORMATS[name]
    n, p, q = 1025, 256, 256
    xa, xb = _x(n, p, 1), _x(n, q, 2)
    a, b = fmt.rows(xa), fmt.rows(xb)
    want = ops.gemm_tn(a, b, p, q, hl=True) if name == "hl" else ops.gemm_tn(a, b, p, q, (p, 2 * p), (q, 2 * q))
    got = fmt.tn(a, b, p, q)
    assert tuple(got.shape) == (p, q) and torch.equal(got, want)
