"""Every launched form of the GEMM tile kernels (csrc/gemm.hip) over the table of tests/gemm_forms.py: edge shapes x K-step states x every
act and output, walk shapes (a workgroup walking two and three tiles through all of full -> full, full -> partial, partial -> full and
partial -> partial), the split-K second launch plain against split, the skinny kernel's K shares -- every element against an fp64
contraction of the operands the kernel was given, within a derived elementwise bound; every output inside guard bands that must stay
intact; every case run twice, bit-identical.  Prints max(err / bound) per (entry, output, act, state): profiles/gemm_forms.txt."""
import ctypes

import pytest
import torch

from tests import gemm_forms as GF

pytestmark = pytest.mark.gpu
DEV = "cuda"
DROPOUT = (0.25, 1234, 77)                   # (p, seed, offset)
LN_EPS = 1e-6


def _ops():
    from snuffy_amd import ops
    return ops


def _true_k(e, k):
    return k // 3 if e.operands == "x3" else k


def _image_cols(out, n):
    return 3 * n if out == "split3" else 2 * n if out == "hl" else n


def _out_dtype(out):
    return torch.float32 if out.startswith("f32") else torch.bfloat16


class Case:
    """One (entry, shape): operands as the kernel takes them, the fp64 contraction, and what the entry needs besides."""

    def __init__(self, name, m, n, k, mark=0):
        ops = _ops()
        self.e = e = GF.ENTRIES[name]
        self.m, self.n, self.k, self.kt = m, n, k, _true_k(e, k)
        self.op = op = GF.operands(m, n, self.kt, bn=mark, device=DEV)
        self.a, self.w, av, wv = GF.kernel_operands(e, op)
        self.bias, self.resid = op.bias, GF.pitched(op.resid)
        self.mask = self.gate = self.stats = self.colsum = None
        if name == "gemm_bf16_lnfold":
            # the kernel's own arithmetic in fp64: rounded operands, the (mean, rstd) and column sums it is handed
            x = op.a.double()
            mean, rstd = x.mean(1), (x.var(1, unbiased=False) + LN_EPS).rsqrt()
            self.stats = torch.stack((mean, rstd), 1).float().contiguous()
            self.colsum = wv.sum(1).float()
            mean, rstd, cs = self.stats[:, 0].double(), self.stats[:, 1].double(), self.colsum.double()
            r = GF.contraction(av, wv)
            p = rstd[:, None] * (r.p - mean[:, None] * cs) + op.bias.double()
            s = rstd[:, None] * (r.s + mean.abs()[:, None] * cs.abs()) + op.bias.double().abs()
            self.r = GF.Reference(p, s)
        else:
            self.r = GF.contraction(av, wv, None if name == "gemm_hl_gated" else op.bias)
        if name in ("gemm_bf16_dropout", "gemm_hl_dropout"):
            self.mask = ops.dropout_mask(1, m, n, *DROPOUT, DEV)[0]
        if name == "gemm_hl_gated":
            g = torch.Generator().manual_seed(m + n)
            act = torch.relu(torch.randn(m, n, generator=g)).to(DEV)
            self.gate = GF.pitched(GF.image_hl(act))
            self.mask = (act.to(torch.bfloat16) > 0).float()

    def launch(self, width, out, act, plain_entry=False):
        """One call into fresh guarded outputs -> [Guarded].  plain_entry: the same shape through the entry's undropped / ungated form."""
        ops, lib, e, m, n, k = _ops(), GF.lib(), self.e, self.m, self.n, self.k
        name = e.name if not plain_entry else {"gemm_bf16_dropout": "gemm_bf16", "gemm_hl_dropout": "gemm_hl", "gemm_hl_gated": "gemm_hl"}[e.name]
        bias = None if e.name == "gemm_hl_gated" else self.bias
        resid = self.resid if out == "f32+resid" else None
        if name == "gemm_bf16_resid_":
            x = GF.Guarded(m, n, torch.float32, rows_only=True, fill=self.op.resid)
            xb = GF.Guarded(m, n, torch.bfloat16, rows_only=True)
            part = GF.Guarded(m, 2 * (n // 32), torch.float32, rows_only=True)
            ops.gemm_bf16_resid_(x.view, self.a, self.w, bias, xb.view, part.view.view(m, n // 32, 2))
            return [x, xb, part]
        g = GF.Guarded(m, _image_cols(out, n), _out_dtype(out))
        c, ldc = ops._p(g.view), g.view.stride(0)
        if name == "gemm_bf16":
            ops.gemm_bf16(self.a, self.w, bias, act, out=g.view, tile_n=width, split3=out == "split3", hl_out=out == "hl")
        elif name in ("gemm_bf16_resid_f32", "gemm_x3_resid_f32"):
            assert ops.gemm_x3(self.a, self.w, bias, act, out=g.view, resid=resid) is g.view
        elif name == "gemm_bf16_dropout":
            rc = lib.snf_gemm_bf16_dropout(ops._p(self.a), self.a.stride(0), ops._p(self.w), self.w.stride(0), ops._p(bias), m, n, k,
                                           ops.ACT_CODES[act], c, ldc, ops.DT_BF16, width, DROPOUT[0], DROPOUT[1], DROPOUT[2], ops._stream())
            assert rc == 0, lib.snf_last_error()
        elif name == "gemm_bf16_lnfold":
            ops.gemm_bf16_lnfold(self.a, self.w, self.colsum, bias, self.stats, act, out=g.view)
        elif name == "gemm_hl":
            ops.gemm_hl(self.a, self.w, bias, act, out=g.view, hl_out=out == "hl", resid=resid)
        elif name == "gemm_hl_dropout":
            ops.gemm_hl_dropout(self.a, self.w, bias, DROPOUT, act, hl_out=out == "hl", resid=resid, out=g.view)
        elif name == "gemm_hl_gated":
            rc = lib.snf_gemm_hl_gated_bf16(ops._p(self.a), self.a.stride(0), ops._p(self.w), self.w.stride(0), ops._p(self.gate),
                                            self.gate.stride(0), m, n, k, c, ldc, ops._stream())
            assert rc == 0, lib.snf_last_error()
        else:
            raise KeyError(name)
        return [g]

    def run(self, width, out, act, tag):
        """Twice, bit-identical, guard bands intact -> the first run's outputs."""
        first, again = self.launch(width, out, act), self.launch(width, out, act)
        for g, h in zip(first, again):
            g.intact(tag)
            assert torch.equal(g.raw, h.raw), tag + ": two runs differ"
        return first

    def check(self, width, out, act, tag):
        """-> max(err / bound) over the outputs of one form at this case."""
        e, n, kt = self.e, self.n, self.kt
        got = self.run(width, out, act, tag)
        resid = self.op.resid if out == "f32+resid" else None
        rounded = out == "bf16"
        if e.name == "gemm_bf16_resid_":
            x, xb, part = (g.view for g in got)
            ref, bound = GF.expected(self.r, e.cls, kt, "none", resid=self.op.resid)
            ratio = GF.check(tag, x, ref, bound, GF.GATE_BF16_F32)
            assert torch.equal(xb, x.to(torch.bfloat16)), tag + ": the bf16 copy is not the rounded new x"
            return max(ratio, GF.check_moments(tag, part.view(self.m, n // 32, 2), x))
        ref, bound = GF.expected(self.r, e.cls, kt, act, resid=resid, mask=self.mask, rounded=rounded)
        if out in ("split3", "hl"):
            # the fp32 value the image is the split of: the fp32-output run of the same form (x the mask tensor, bit for bit)
            if e.name in ("gemm_hl_dropout", "gemm_hl_gated"):
                value = self.launch(width, "f32", act, plain_entry=True)[0].view * self.mask
            else:
                value = self.launch(width, "f32", act)[0].view
            return GF.check_image(tag, out, got[0].view, n, value, ref, bound, GF.GATE_BF16_OUT, GF.gate_of(e, False))
        return GF.check(tag, got[0].view, ref, bound, GF.gate_of(e, rounded))


def _report(name, out, act, state, ratio):
    print("gemm_forms | %-22s | %-9s | %-9s | %-30s | %.4f" % (name, out, act, state, GF.record(name, out, act, state, ratio)))


# ---- edge shapes x K-step states x every act and output of every entry ------------------------------------------------------------------------------
EDGE_PARAMS = [(name, w, o, a) for name in GF.TILE_ENTRIES for e in [GF.ENTRIES[name]] for w in e.widths for o in e.outs
               for a in GF.out_acts(e, o)]


@pytest.fixture
def plain_walk(monkeypatch):
    """gemm_hl's plain form: no split-K second launch (no edge or walk shape has 16 K steps, the switch is for the record)."""
    monkeypatch.setattr(_ops(), "GEMM_HL_SPLITK", False)


@pytest.mark.parametrize("name,width,out,act", EDGE_PARAMS, ids=["-".join(map(str, p)) for p in EDGE_PARAMS])
def test_edge_shapes_at_every_k_step_state(name, width, out, act, plain_walk):
    e = GF.ENTRIES[name]
    cases = [(m, n, k) for w, o, a, m, n, k in GF.edge_cases(e) if (w, o, a) == (width, out, act)]
    assert cases
    worst = {}
    for m, n, k in cases:
        ratio = Case(name, m, n, k).check(width, out, act, "%s %s %s w%d (%d, %d, %d)" % (name, out, act, width, m, n, k))
        worst[k] = max(worst.get(k, 0.0), ratio)
    for k, ratio in sorted(worst.items()):
        _report(name, out + ("/%d" % width if len(e.widths) > 1 else ""), act, "edge k=%d" % k, ratio)


# ---- walk shapes --------------------------------------------------------------------------------------------------------------------------------------
def _walk_params():
    seen = []
    for name in GF.TILE_ENTRIES:
        for w, o, a, L, m, n, k in GF.walk_cases(GF.ENTRIES[name], 256):
            if (name, w, o, L) not in seen:
                seen.append((name, w, o, L))
    return seen


WALK_PARAMS = _walk_params()


@pytest.mark.parametrize("name,width,out,length", WALK_PARAMS, ids=["-".join(map(str, p)) for p in WALK_PARAMS])
def test_walk_shapes_reach_every_transition(name, width, out, length, plain_walk):
    e = GF.ENTRIES[name]
    cus = GF.cu_count()
    cases = [(a, m, n, k) for w, o, a, L, m, n, k in GF.walk_cases(e, cus) if (w, o, L) == (width, out, length)]
    assert cases
    for act, m, n, k in cases:
        bn = width or 256
        st = GF.walk_states(m, n, bn, cus)
        assert st.transitions == {"FF", "FP", "PF", "PP"} and st.lengths == {length - 1, length}, (m, n, bn, cus, st)
        launch_width = 0 if name == "gemm_bf16_resid_" else width
        tag = "%s %s %s w%d (%d, %d, %d) walk %d" % (name, out, act, width, m, n, k, length)
        ratio = Case(name, m, n, k, mark=bn).check(launch_width, out, act, tag)
        _report(name, out + ("/%d" % width if len(e.widths) > 1 or name == "gemm_bf16_resid_" else ""), act,
                "walk %d-%d k=%d m=%d" % (length - 1, length, k, m), ratio)


# ---- the split-K second launch ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def split_case():
    """One split shape's operands and contraction at a time (the largest is 22400 x 768 x 1024)."""
    cache = {}

    def get(shape):
        if shape not in cache:
            cache.clear()
            torch.cuda.empty_cache()
            cache[shape] = Case("gemm_hl_split", *shape)
        return cache[shape]
    return get


def _hl_outputs(case, out, act, dropout=False):
    """ops.gemm_hl / gemm_hl_dropout of a split case into a guarded output, twice, bit-identical -> the output view."""
    ops = _ops()
    runs = []
    for _ in range(2):
        g = GF.Guarded(case.m, _image_cols(out, case.n), _out_dtype(out))
        kw = dict(out=g.view, hl_out=out == "hl", resid=case.resid if out == "f32+resid" else None)
        if dropout:
            ops.gemm_hl_dropout(case.a, case.w, case.bias, DROPOUT, act, **kw)
        else:
            ops.gemm_hl(case.a, case.w, case.bias, act, **kw)
        g.intact("split %s %s" % (out, act))
        runs.append(g)
    assert torch.equal(runs[0].raw, runs[1].raw)
    return runs[0].view


def _decoded(view, out, n):
    if out != "hl":
        return view.double()
    hi, lo = GF.decode_hl(view, n)
    return hi.double() + lo.double()


@pytest.mark.parametrize("act", GF.ENTRIES["gemm_hl_split"].acts)
@pytest.mark.parametrize("shape", GF.SPLIT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_split_k_against_plain_and_fp64(shape, act, split_case, monkeypatch):
    ops, e = _ops(), GF.ENTRIES["gemm_hl_split"]
    m, n, k = shape
    cus = GF.cu_count()
    geo = GF.split_geometry(m, n, k, cus)
    assert geo.ws_bytes == GF.lib_ws_bytes(m, n, k) and bool(geo.tiles) == (shape != (900, 768, 480))
    case = split_case(shape)
    for out in e.outs:
        if out == "hl" and n % 32:
            continue
        resid = case.op.resid if out == "f32+resid" else None
        ref, bound = GF.expected(case.r, "fp32", k, act, resid=resid, rounded=out == "bf16")
        if out == "hl":
            bound = bound + 2.0 ** -16 * ref.abs()
        monkeypatch.setattr(ops, "GEMM_HL_SPLITK", True)
        split = _hl_outputs(case, out, act)
        if geo.ws_bytes:
            # the scratch comes from the allocator per call and may be dirty: the call zeroes its own tickets
            junk = torch.full((geo.ws_bytes,), 0xAB, dtype=torch.uint8, device=DEV)
            del junk
            assert torch.equal(split, _hl_outputs(case, out, act)), "dirty workspace"
        monkeypatch.setattr(ops, "GEMM_HL_SPLITK", False)
        plain = _hl_outputs(case, out, act)
        tag = "gemm_hl %s %s %s" % (shape, out, act)
        gate = GF.GATE_BF16_OUT if out == "bf16" else GF.GATE_X3_F32
        r_split = GF.check(tag + " split", _decoded(split, out, n), ref, bound, gate)
        r_plain = GF.check(tag + " plain", _decoded(plain, out, n), ref, bound, gate)
        scale = max(1.0, float(ref.abs().max()))
        if out == "f32+resid":
            assert float((split - plain).abs().max()) <= 2e-6 * scale
        if not geo.tiles:
            assert torch.equal(split, plain)
        else:
            # outside the split tiles both launches ran the same code
            same = torch.ones(-(-m // 256), -(-n // 256), dtype=torch.bool)
            for t in geo.tiles:
                same[t // same.shape[1], t % same.shape[1]] = False
            cols = 2 * 256 if out == "hl" else 256
            for tm, tn in same.nonzero().tolist()[:: max(1, int(same.sum()) // 16)]:
                assert torch.equal(split[256 * tm:256 * (tm + 1), cols * tn:cols * (tn + 1)], plain[256 * tm:256 * (tm + 1), cols * tn:cols * (tn + 1)])
        _report("gemm_hl_split", out, act, "%dx%dx%d parts %s" % (m, n, k, sorted(set(geo.tiles.values())) or "-"), r_split)
        _report("gemm_hl", out, act, "%dx%dx%d plain" % shape, r_plain)


@pytest.mark.parametrize("shape", GF.SPLIT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_split_k_with_dropout(shape, split_case, monkeypatch):
    ops = _ops()
    m, n, k = shape
    case = split_case(shape)
    mask = ops.dropout_mask(1, m, n, *DROPOUT, DEV)[0]
    for out, act in (("hl", "relu"), ("f32+resid", "none")):
        if out == "hl" and n % 32:
            continue
        ref, bound = GF.expected(case.r, "fp32", k, act, resid=case.op.resid if out == "f32+resid" else None, mask=mask)
        if out == "hl":
            bound = bound + 2.0 ** -16 * ref.abs()
        res = {}
        for on in (True, False):
            monkeypatch.setattr(ops, "GEMM_HL_SPLITK", on)
            res[on] = _hl_outputs(case, out, act, dropout=True)
            ratio = GF.check("gemm_hl_dropout %s %s split=%s" % (shape, out, on), _decoded(res[on], out, n), ref, bound, GF.GATE_X3_F32)
            _report("gemm_hl_dropout", out, act, "%dx%dx%d %s" % (m, n, k, "split" if on else "plain"), ratio)
        if out == "f32+resid":
            assert float((res[True] - res[False]).abs().max()) <= 2e-6 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("shape", [s for s in GF.SPLIT_SHAPES if s != (900, 768, 480)], ids=lambda s: "x".join(map(str, s)))
def test_deferred_split(shape, split_case):
    """snf_gemm_hl_deferred_f32 through its C entry with own buffers: z + DeferredK.add_to against the reference, the map non-zero exactly at
    the tiles split_geometry names, z inside guard bands, the workspace's tail untouched, two runs bit-identical (z, map and slabs)."""
    ops, lib = _ops(), GF.lib()
    m, n, k = shape
    case = split_case(shape)
    geo = GF.split_geometry(m, n, k, GF.cu_count())
    nbytes, off = GF.lib_deferred_bytes(m, n, k)
    assert (nbytes, off) == (geo.deferred_bytes, geo.slab_offset) and nbytes
    tm, tn = -(-m // 256), -(-n // 256)
    runs = []
    for _ in range(2):
        z = GF.Guarded(m, n, torch.float32)
        ws = torch.full((nbytes + 4096,), 0x5A, dtype=torch.uint8, device=DEV)
        rc = lib.snf_gemm_hl_deferred_f32(ops._p(case.a), case.a.stride(0), ops._p(case.w), case.w.stride(0), ops._p(case.bias),
                                          ops._p(case.resid), case.resid.stride(0), m, n, k, ops.ACT_CODES["none"], ops._p(z.view),
                                          z.view.stride(0), ops.DT_F32, ops._p(ws), nbytes, ops._stream())
        assert rc == 0, lib.snf_last_error()
        z.intact("deferred z")
        assert bool((ws[nbytes:] == 0x5A).all()), "deferred: workspace written past its size"
        runs.append((z, ws))
    (z, ws), (z2, ws2) = runs
    assert torch.equal(z.raw, z2.raw) and torch.equal(ws, ws2)
    tile_map = ws[:4 * tm * tn].view(torch.int32).view(tm, tn)
    assert sorted(int(a) * tn + int(b) for a, b in tile_map.nonzero().tolist()) == sorted(geo.tiles)
    assert sorted(tile_map[tile_map > 0].tolist()) == sorted(set(tile_map[tile_map > 0].tolist())) and int(tile_map.max()) <= 8 * geo.rcap
    slabs = ws[off:nbytes].view(torch.float32).view(-1, 256, 256)
    total = ops.DeferredK(slabs, tile_map, ws).add_to(z.view)
    ref, bound = GF.expected(case.r, "fp32", k, "none", resid=case.op.resid)
    _report("gemm_hl_deferred", "f32+resid", "none", "%dx%dx%d" % shape, GF.check("deferred %s" % (shape,), total, ref, bound, GF.GATE_X3_F32))


# ---- the skinny kernel ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out", ["f32", "bf16", "f32pair"])
@pytest.mark.parametrize("k", GF.K_SKINNY)
def test_skinny_kernel_k_shares(k, out):
    ops, lib = _ops(), GF.lib()
    name = "linear_rows_x3_resid" if out == "f32pair" else "linear_rows_x3"
    e = GF.ENTRIES[name]
    worst = 0.0
    for r in GF.R_SKINNY:
        for c in GF.C_SKINNY:
            op = GF.operands(r, c, k, device=DEV)
            x, w = GF.pitched(op.a), GF.pitched(op.w)
            resid = GF.pitched(op.resid)
            for bias in (op.bias, None):
                con = GF.contraction(op.a.double(), op.w.double(), bias)
                runs = []
                for _ in range(2):
                    g = [GF.Guarded(r, c, torch.bfloat16 if out == "bf16" else torch.float32) for _ in range(2 if out == "f32pair" else 1)]
                    if out == "f32pair":
                        rc = lib.snf_linear_rows_x3_resid_f32(ops._p(x), x.stride(0), ops._p(w), w.stride(0), ops._p(bias), ops._p(resid),
                                                              resid.stride(0), r, c, k, ops._p(g[0].view), g[0].view.stride(0),
                                                              ops._p(g[1].view), g[1].view.stride(0), ops._stream())
                    else:
                        rc = lib.snf_linear_rows_x3_f32(ops._p(x), x.stride(0), ops._p(w), w.stride(0), ops._p(bias), r, c, k, ops._p(g[0].view),
                                                        g[0].view.stride(0), ops.DT_BF16 if out == "bf16" else ops.DT_F32, ops._stream())
                    assert rc == 0, lib.snf_last_error()
                    runs.append(g)
                tag = "%s %s r=%d c=%d k=%d bias=%s" % (name, out, r, c, k, bias is not None)
                for g, h in zip(*runs):
                    g.intact(tag)
                    assert torch.equal(g.raw, h.raw), tag
                ref, bound = GF.expected(con, "fp32", k, "none", rounded=out == "bf16")
                worst = max(worst, GF.check(tag, runs[0][0].view, ref, bound, GF.gate_of(e, out == "bf16")))
                if out == "f32pair":
                    ref, bound = GF.expected(con, "fp32", k, "none", resid=op.resid)
                    worst = max(worst, GF.check(tag + " out2", runs[0][1].view, ref, bound, GF.GATE_SKINNY_F32))
    _report(name, out, "none", "k=%d (%d steps)" % (k, k // 16), worst)
