"""The launched forms of the GEMM tile kernels (csrc/gemm.hip: gemm_bf16_kernel, gemm_hl_kernel, skinny_linear_x3_kernel), as the tests see
them: one record per instantiation family with what it admits, the tile -> XCD -> workgroup walk and the split-K geometry restated in
Python, the shapes that reach every walk state / K-step state / store predicate, and the operands, guard bands, fp64 references, derived
elementwise bounds and checkers the form tests share.  Plain data and helpers, no test functions: test_gemm_forms_host.py proves the
table complete and the checkers sharp (no device needed), test_gpu_gemm_forms.py runs it.

Bounds are derived (see bound_eps), never measured; next to them stand the project's max-norm gates, as literals from test_gpu_gemm.py."""
import collections
import ctypes
import math

import torch
import torch.nn.functional as F

from tests.helpers import _ops, _split_host

BM = 256
ACTS = ("none", "relu", "leakyrelu", "gelu", "selu")
LINE_ACTS, DIRECT_ACTS = ("none", "relu", "leakyrelu"), ("gelu", "selu")       # store class: LDS line-store transposes / direct stores


def store_class(act):
    return "line" if act in LINE_ACTS else "direct"


# ---- K-step states ---------------------------------------------------------------------------------------------------------------------------
# gemm_bf16_kernel (ring of NBUF = 4 step buffers, DMA AHEAD = 2 steps): 64 ns == AHEAD, every in-loop stage belongs to the next tile;
# 96 one in-tile stage; 128 ns == NBUF; 160 the ring wraps inside a tile; 288 nine steps, the ring phase differs from tile to tile
K_BF16 = (64, 96, 128, 160, 288)
K_EPI = (96, 128, 160, 288)                 # the EPI forms start at AHEAD + 1 steps
K_HL = (32, 64, 96, 160)                    # gemm_hl_kernel (two buffers, one step ahead): one, two, three, five steps
K_SKINNY = (16, 32, 48, 144, 800, 768)      # 8 waves x batches of 6 16-deep steps: fewer steps than waves; an uneven share; 7 steps per wave
R_SKINNY, C_SKINNY = (1, 31, 33, 224), (1, 33, 100, 768)

# ---- edge shapes: one tile per workgroup, ragged both ways, every store predicate live --------------------------------------------------------
EDGE = ((300, 264), (257, 8), (1, 136), (255, 392), (512, 512))
EDGE_32 = ((300, 288), (1, 160), (512, 512))                  # forms that need n % 32
EDGE_64 = ((300, 320), (257, 64), (300, 448), (512, 512))     # forms that need n % 64

# ---- walk shapes: n = 576 is three ragged 256-wide / five ragged 128-wide column tiles and a multiple of 64; 704 the 256-wide EPI 2 form --------
WALK_N, WALK_N_EPI2_256 = 576, 704
WALK_LENGTHS = (2, 3)                        # the longest walk; no walk shorter than one less
WALK_ACTS = ("none", "gelu")                 # one act per store class

# ---- split shapes (m, n, k) of the gemm_hl second launch -----------------------------------------------------------------------------------------
SPLIT_SHAPES = ((900, 768, 544), (22400, 768, 800), (22400, 768, 1024), (900, 768, 480), (33000, 520, 1024))
HL_SPLIT_MIN_STEPS, HL_SPLIT_MAX, HL_TICKET_BYTES = 8, 4, 4096

Entry = collections.namedtuple("Entry", "name kernel cls operands widths outs acts min_k gran ks")
# cls: which arithmetic class bounds it; operands: bf16 | x3 ([hi | hi | lo] images) | hl (interleaved images) | f32;
# widths: tile_n values (0 = the entry's own rule); gran: the granule of n
ENTRIES = collections.OrderedDict((e.name, e) for e in (
    Entry("gemm_bf16", "gemm_bf16_kernel<NI,ACT,OUT,0,MI>", "bf16", "bf16", (256, 128), ("bf16", "f32", "split3", "hl"), ACTS, 64, 8, K_BF16),
    Entry("gemm_bf16_resid_f32", "gemm_bf16_kernel + P.resid", "bf16", "bf16", (0,), ("f32+resid",), ACTS, 64, 8, K_BF16),
    Entry("gemm_x3_resid_f32", "gemm_bf16_kernel + P.resid", "fp32", "x3", (0,), ("f32+resid",), ACTS, 64, 8, (96, 288)),
    Entry("gemm_bf16_dropout", "gemm_bf16_kernel<..,DROP>", "bf16", "bf16", (256, 128), ("bf16",), ("relu",), 64, 8, K_BF16),
    Entry("gemm_bf16_lnfold", "gemm_bf16_kernel<4,ACT,0,1>", "bf16", "bf16", (256,), ("bf16",), ("none", "gelu"), 96, 64, K_EPI),
    Entry("gemm_bf16_resid_", "gemm_bf16_kernel<NI,NONE,1,2>", "bf16", "bf16", (0,), ("epi2",), ("none",), 96, 64, K_EPI),
    Entry("gemm_hl", "gemm_hl_kernel<ACT,OUT>", "fp32", "hl", (256,), ("f32", "f32+resid", "bf16", "hl"), ACTS, 32, 8, K_HL),
    Entry("gemm_hl_split", "gemm_hl_kernel<ACT,OUT,1>", "fp32", "hl", (256,), ("f32+resid", "bf16", "hl"), ("none", "relu", "gelu"), 512, 8, ()),
    Entry("gemm_hl_dropout", "gemm_hl_kernel<..,DROP>", "fp32", "hl", (256,), ("hl", "f32+resid"), ("relu", "none"), 32, 8, K_HL),
    Entry("gemm_hl_deferred", "gemm_hl_kernel<NONE,1,2>", "fp32", "hl", (256,), ("f32+resid",), ("none",), 512, 8, ()),
    Entry("gemm_hl_gated", "gemm_hl_kernel<NONE,3,0,GATE>", "fp32", "hl", (256,), ("hl",), ("none",), 32, 32, K_HL),
    Entry("linear_rows_x3", "skinny_linear_x3_kernel", "fp32", "f32", (32,), ("f32", "bf16"), ("none",), 16, 1, K_SKINNY),
    Entry("linear_rows_x3_resid", "skinny_linear_x3_kernel", "fp32", "f32", (32,), ("f32pair",), ("none",), 16, 1, K_SKINNY),
))
TILE_ENTRIES = [n for n, e in ENTRIES.items() if e.ks and e.operands != "f32"]       # the ones that walk tiles at edge and walk shapes


def out_acts(entry, out):
    """The acts an (entry, output) pair exists for: gemm_hl_dropout is relu -> hl image and none -> fp32 + resid."""
    if entry.name == "gemm_hl_dropout":
        return ("relu",) if out == "hl" else ("none",)
    return entry.acts


def out_gran(entry, out):
    return max(entry.gran, 32 if out == "hl" else 8)


def edge_shapes(entry, out):
    g = out_gran(entry, out)
    return EDGE_64 if g == 64 else EDGE_32 if g == 32 else EDGE


def tile_width(entry, width, m, n, cus):
    """The tile width a launch takes: the asked one, or the entry's own rule (gemm.hip: gemm_bf16_impl, snf_gemm_bf16_resid)."""
    if width:
        return width
    if entry.name == "gemm_bf16_resid_":
        return 128 if 1 <= n % 256 <= 128 else 256
    t256 = -(-m // BM) * -(-n // 256)
    return 256 if n > 128 and t256 * 10 >= cus * 7 else 128


def edge_cases(entry):
    """[(width, out, act, m, n, k)]: edge shapes x K-step states x every act and output of the entry."""
    return [(w, o, a, m, n, k) for w in entry.widths for o in entry.outs for a in out_acts(entry, o) for m, n in edge_shapes(entry, o)
            for k in entry.ks]


def walk_ks(entry):
    return (32, 96) if entry.operands == "hl" else (entry.ks[0],)


def walk_n(entry, width):
    return WALK_N_EPI2_256 if entry.name == "gemm_bf16_resid_" and width == 256 else WALK_N


def walk_cases(entry, cus):
    """[(width, out, act, length, m, n, k)]: walk shapes x {none, gelu} x every (width, output) of the entry.  An entry that picks its own
    width is listed at the widths its rule gives the walk shapes."""
    cases = []
    for w in ((256, 128) if entry.name == "gemm_bf16_resid_" else entry.widths):
        for o in entry.outs:
            for a in [a for a in WALK_ACTS if a in out_acts(entry, o)] or out_acts(entry, o):
                for length in WALK_LENGTHS:
                    n = walk_n(entry, w)
                    bn = w or 256
                    m = walk_rows(n, bn, cus, length)
                    assert tile_width(entry, 0 if entry.name == "gemm_bf16_resid_" else w, m, n, cus) == bn
                    cases += [(w, o, a, length, m, n, k) for k in walk_ks(entry)]
    return cases


# ---- the walk, restated (gemm.hip: the tile stream of both tile kernels and the grid rule of launch / launch_hl) ---------------------------------
def grid_of(ntiles, cus):
    grid = max(cus & ~7, 8)
    return min(grid, 8 * -(-ntiles // 8))


def xcd_range(ntiles, xcd):
    q, r = ntiles >> 3, ntiles & 7
    lo = xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q
    return lo, lo + q + (1 if xcd < r else 0)


def walk(m, n, bn, cus):
    """{workgroup (blockIdx.x): [(tile, full)]}: workgroup b runs on XCD b % 8, every XCD owns a contiguous range of tiles and its workgroups
    take them round robin.  A tile is full where no row and no column of it lies past the matrix."""
    tiles_m, tiles_n = -(-m // BM), -(-n // bn)
    ntiles = tiles_m * tiles_n
    grid = grid_of(ntiles, cus)
    per = grid >> 3
    out = {}
    for b in range(grid):
        lo, hi = xcd_range(ntiles, b & 7)
        seq = []
        for t in range(lo + (b >> 3), hi, per):
            tm, tn = divmod(t, tiles_n)
            seq.append((t, (tm + 1) * BM <= m and (tn + 1) * bn <= n))
        if seq:
            out[b] = seq
    return out


WalkStates = collections.namedtuple("WalkStates", "transitions first last lengths")


def walk_states(m, n, bn, cus):
    """The transitions {FF, FP, PF, PP} between consecutive tiles of one workgroup, the kinds of first and last tiles, the walk lengths."""
    tr, first, last, lengths = set(), set(), set(), set()
    for seq in walk(m, n, bn, cus).values():
        kinds = ["F" if f else "P" for _, f in seq]
        tr.update(a + b for a, b in zip(kinds, kinds[1:]))
        first.add(kinds[0]), last.add(kinds[-1]), lengths.add(len(kinds))
    return WalkStates(tr, first, last, lengths)


def walk_rows(n, bn, cus, length):
    """The smallest m = 256 t + 37 whose longest walk is `length`, with no walk shorter than length - 1 and all four transitions."""
    for t in range(0, 4096):
        m = 256 * t + 37
        ntiles = (t + 1) * -(-n // bn)
        per = grid_of(ntiles, cus) >> 3
        longest = -(-(-(-ntiles // 8)) // per)
        if longest < length:
            continue
        if longest > length:
            break
        st = walk_states(m, n, bn, cus)
        if max(st.lengths) == length and min(st.lengths) >= length - 1 and st.transitions == {"FF", "FP", "PF", "PP"}:
            return m
    raise ValueError("no row count walks %d tiles at n=%d bn=%d on %d CUs" % (length, n, bn, cus))


# ---- the split geometry, restated (gemm.hip: hl_split_geometry, hl_deferred_geometry and the kernel's own per-XCD rule) ----------------------------
SplitGeometry = collections.namedtuple("SplitGeometry", "cap rcap xcds ws_bytes deferred_bytes slab_offset tiles")
# xcds: per XCD (q tiles, r tiles of the last round, parts per such tile; 1 = not split); tiles: {tile: parts} of the split tiles


def split_geometry(m, n, k, cus):
    none = SplitGeometry(0, 0, (), 0, 0, 0, {})
    if m < 1 or n < 1 or k < 32:
        return none
    ntiles, ns = -(-m // BM) * -(-n // 256), k // 32
    grid = grid_of(ntiles, cus)
    w = grid >> 3
    if ntiles > 2 * grid:
        return none
    cap = rcap = 0
    per_xcd = []
    for x in range(8):
        lo, hi = xcd_range(ntiles, x)
        q = hi - lo
        r = q % w
        sn = min(w // r, HL_SPLIT_MAX, ns // HL_SPLIT_MIN_STEPS) if r else 0
        per_xcd.append((q, r, sn if sn >= 2 else 1))
        if sn >= 2:
            cap, rcap = max(cap, sn), max(rcap, r)
    if cap < 2 or 8 * rcap * 4 > HL_TICKET_BYTES:
        # (the library sizes no workspace where the tickets would not fit their 4 KiB; no shape of the table comes near)
        return none._replace(xcds=tuple((q, r, 1) for q, r, _ in per_xcd))
    tiles = {}
    for x, (q, r, parts) in enumerate(per_xcd):
        if parts >= 2:
            lo, hi = xcd_range(ntiles, x)
            for t in range(hi - r, hi):
                tiles[t] = parts
    ws = HL_TICKET_BYTES + 8 * rcap * cap * BM * 256 * 4
    map_rcap = max(-(-ntiles // 8), rcap)
    slab_offset = (8 * map_rcap * 4 + 4095) & ~4095
    return SplitGeometry(cap, rcap, tuple(per_xcd), ws, slab_offset + 8 * rcap * BM * 256 * 4, slab_offset, tiles)


def part_steps(ns, parts):
    return [(p + 1) * ns // parts - p * ns // parts for p in range(parts)]


# ---- the library's own figures -----------------------------------------------------------------------------------------------------------------
def lib():
    return _ops()._ffi.load()


def cu_count():
    return int(lib().snf_device_cu_count())


def lib_ws_bytes(m, n, k):
    return int(lib().snf_gemm_hl_ws_bytes(m, n, k))


def lib_deferred_bytes(m, n, k):
    off = ctypes.c_size_t(0)
    return int(lib().snf_gemm_hl_deferred_ws_bytes(m, n, k, ctypes.byref(off))), int(off.value)


# ---- operands ----------------------------------------------------------------------------------------------------------------------------------
PAD = 64                                                    # NaN columns behind every operand row: a step that reads past k poisons its tile
Operands = collections.namedtuple("Operands", "a w bias resid")
_cache = {}


def operands(m, n, k, bn=0, device="cuda", want_resid=True):
    """fp32 a ~ N(0, 1) [m, k], w ~ N(0, 1) / sqrt(k) [n, k], bias, resid ~ N(0, 1), seeded on the CPU generator.  bn (walk shapes): the
    element's tile coordinates tm + 3 tn ride on column 0 of a (tm) and on the bias (3 tn): a tile computed from its neighbour's operands
    or bias differs by O(1) in every element.  One set is kept alive at a time."""
    key = (m, n, k, bn, str(device), want_resid)
    if key not in _cache:
        _cache.clear()
        g = torch.Generator().manual_seed((m * 7919 + n * 104729 + k) % (2 ** 31))
        a = torch.randn(m, k, generator=g)
        w = torch.randn(n, k, generator=g) / k ** 0.5
        bias = torch.randn(n, generator=g)
        resid = torch.randn(m, n, generator=g) if want_resid else None
        if bn:
            a[:, 0] += (torch.arange(m) // BM).float()
            w[:, 0] = w[:, 0].abs() + 0.5                  # ... and every column sees the row coordinate with weight >= 0.5
            bias += 3.0 * (torch.arange(n) // bn).float()
            # Column 0 holds bf16 values (lo = 0 in a split image, the product exact in fp32).  Its one product is up to 100 x the sum of
            # the others: carrying the 2^-17 of its own split it alone set the fp32-class error (1.6e-5 of the result scale at tm = 90,
            # k = 32, inside the elementwise bound but past the 8e-6 max-norm gate, which stands for k comparable terms) -- an error
            # that says nothing about the walk the mark is there for.
            a[:, 0], w[:, 0] = a[:, 0].to(torch.bfloat16).float(), w[:, 0].to(torch.bfloat16).float()
        _cache[key] = Operands(a.to(device), w.to(device), bias.to(device), None if resid is None else resid.to(device))
    return _cache[key]


def pitched(t, pad=PAD):
    """t as the [:, :cols] view of a buffer `pad` columns wider, the padding NaN."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), dtype=t.dtype, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


def image_hl(x):
    """[m, 2 k] bf16 of fp32 x [m, k]: every 32 columns as [hi(32) | lo(32)]."""
    hi, lo = _split_host(x)
    m, k = x.shape
    return torch.stack((hi.view(m, k // 32, 32), lo.view(m, k // 32, 32)), 2).reshape(m, 2 * k)


def image_x3(x, weight=False):
    """[hi | hi | lo] of the rows, [Wh | Wl | Wh] of the weight."""
    hi, lo = _split_host(x)
    return torch.cat((hi, lo, hi) if weight else (hi, hi, lo), 1)


def kernel_operands(entry, op):
    """(a, w) as the entry's kernel takes them (pitched views) and (av, wv): the fp64 values the reference contracts -- the bf16-rounded
    operands of a bf16-class form, the fp32 operands of an fp32-class one."""
    if entry.operands == "bf16":
        a, w = op.a.to(torch.bfloat16), op.w.to(torch.bfloat16)
        return pitched(a), pitched(w), a.double(), w.double()
    if entry.operands == "x3":
        return pitched(image_x3(op.a)), pitched(image_x3(op.w, True)), op.a.double(), op.w.double()
    if entry.operands == "hl":
        return pitched(image_hl(op.a)), pitched(image_hl(op.w)), op.a.double(), op.w.double()
    return pitched(op.a), pitched(op.w), op.a.double(), op.w.double()


# ---- guard bands ---------------------------------------------------------------------------------------------------------------------------------
GUARD_ROWS, GUARD_COLS = 8, 64
_SENTINEL = {1: 0x5A, 2: 0x7FA5, 4: 0x7FA5A5A5}             # NaN bit patterns of bf16 and f32: an unwritten element inside the view shows as well
_RAW = {1: torch.uint8, 2: torch.int16, 4: torch.int32}


class Guarded:
    """view = [:m, :cols] of a buffer with 8 more rows and 64 more columns (rows_only: a contiguous view, 8 more rows), pre-filled with a
    sentinel bit pattern; intact() asserts that every byte outside the view still holds it."""

    def __init__(self, m, cols, dtype, device="cuda", rows_only=False, fill=None):
        size = torch.empty(0, dtype=dtype).element_size()
        self.m, self.cols, self.pat = m, cols, _SENTINEL[size]
        self.raw = torch.full((m + GUARD_ROWS, cols + (0 if rows_only else GUARD_COLS)), self.pat, dtype=_RAW[size], device=device)
        self.view = self.raw.view(dtype)[:m, :cols]
        if fill is not None:
            self.view.copy_(fill)

    def intact(self, tag=""):
        below, right = self.raw[self.m:], self.raw[:self.m, self.cols:]
        if not (bool((below == self.pat).all()) and bool((right == self.pat).all())):
            bad = (self.raw != self.pat)
            bad[:self.m, :self.cols] = False
            at = bad.nonzero()[0].tolist()
            raise AssertionError("%s: guard band written at row %d column %d of a [%d, %d] output" % (tag, at[0], at[1], self.m, self.cols))


# ---- fp64 references and the derived elementwise bound -------------------------------------------------------------------------------------------
def bound_eps(cls, k):
    """Relative to S = |a| |w|^T + |bias| (+ |resid|), elementwise.
    bf16 class, fp32 result: (k + 2) 2^-23 -- products of bf16 values are exact in fp32; k additions in any order and either rounding mode, the
    bias and one more rounding are covered.
    fp32 class (split-bf16 x3): 2^-16 + (3 k + 2) 2^-23 -- hi + lo represents either operand to 2^-18 and the dropped lo lo product is below
    2^-18 |a| |w| (three terms, under 2^-16 together); 3 k additions."""
    return (k + 2) * 2.0 ** -23 if cls == "bf16" else 2.0 ** -16 + (3 * k + 2) * 2.0 ** -23


def ref_act(p, act):
    return {"none": lambda t: t, "relu": F.relu, "gelu": F.gelu, "leakyrelu": lambda t: F.leaky_relu(t, 0.01), "selu": F.selu}[act](p)


def act_bound(p, ref, b, act):
    """relu / leakyrelu are Lipschitz 1; gelu 1.13 and the kernel's erf polynomial states 1.5e-7; selu 1.76 (scale x alpha) and one exp2."""
    if act == "gelu":
        return 1.13 * b + 1e-7 * p.abs() + 2.0 ** -21 * ref.abs()
    if act == "selu":
        return 1.76 * b + 2.0 ** -20 * (ref.abs() + 1.76)
    return b


Reference = collections.namedtuple("Reference", "p s")


def contraction(av, wv, bias=None):
    """(P, S): the pre-activation product in fp64 and the sum of the magnitudes it is made of."""
    p, s = av @ wv.t(), av.abs() @ wv.abs().t()
    if bias is not None:
        p, s = p + bias.double(), s + bias.double().abs()
    return Reference(p, s)


def expected(r, cls, k, act, resid=None, mask=None, rounded=False):
    """(ref, bound) of act(P) (x mask) (+ resid); rounded: a bf16 or hi-plane output, one more rounding of 2^-8 |ref|."""
    eps = bound_eps(cls, k)
    ref = ref_act(r.p, act)
    b = act_bound(r.p, ref, eps * r.s, act)
    if mask is not None:
        ref, b = ref * mask.double(), b * mask.double() + 2.0 ** -23 * (ref * mask.double()).abs()
    if resid is not None:
        ref, b = ref + resid.double(), b + eps * resid.double().abs()
    if rounded:
        b = b + 2.0 ** -8 * ref.abs()
    return ref, b


# the project's max-norm gates (test_gpu_gemm.py): bf16 class fp32 out, any bf16 out, fp32 class fp32 out; the skinny kernel's two
GATE_BF16_F32, GATE_BF16_OUT, GATE_X3_F32, GATE_SKINNY_F32, GATE_SKINNY_BF16 = 2e-5, 4.5e-3, 8e-6, 2e-5, 5e-3


def gate_of(entry, rounded):
    if entry.operands == "f32":
        return GATE_SKINNY_BF16 if rounded else GATE_SKINNY_F32
    return GATE_BF16_OUT if rounded else GATE_BF16_F32 if entry.cls == "bf16" else GATE_X3_F32


# ---- the checkers ---------------------------------------------------------------------------------------------------------------------------------
def check(tag, got, ref, bound, gate):
    """Every element finite and within its own bound, and the max error within gate x max(1, max |ref|).  -> max(err / bound)."""
    got = got.double()
    if tuple(got.shape) != tuple(ref.shape):
        raise AssertionError("%s: shape %s, reference %s" % (tag, tuple(got.shape), tuple(ref.shape)))
    finite = torch.isfinite(got)
    if not bool(finite.all()):
        at = (~finite).nonzero()[0].tolist()
        raise AssertionError("%s: not finite at %s (tile %d, %d)" % (tag, at, at[0] // BM, at[1] // 256))
    err = (got - ref).abs()
    over = err > bound
    if bool(over.any()):
        at = over.nonzero()[0].tolist()
        raise AssertionError("%s: %d elements past their bound, first at %s (tile row %d): got %.9g ref %.9g bound %.3g"
                             % (tag, int(over.sum()), at, at[0] // BM, float(got[tuple(at)]), float(ref[tuple(at)]), float(bound[tuple(at)])))
    scale = max(1.0, float(ref.abs().max()))
    if float(err.max()) > gate * scale:
        raise AssertionError("%s: max error %.3e past %.1e x %.3g" % (tag, float(err.max()), gate, scale))
    return float((err / bound.clamp_min(1e-300)).max())


def decode_hl(img, n):
    m = img.shape[0]
    v = img.reshape(m, n // 32, 2, 32)
    return v[:, :, 0].reshape(m, n), v[:, :, 1].reshape(m, n)


def decode_split3(img, n):
    return img[:, :n], img[:, n:2 * n], img[:, 2 * n:]


def check_image(tag, kind, img, n, f32_run, ref, bound, gate_hi, gate_sum):
    """An image output ([hi | hi | lo] or [hi(32) | lo(32)]): hi == bf16(value) bit for bit against the fp32-output run of the same form, hi
    within the rounded bound, and hi + lo against the reference (hi + lo represents a value to 2^-16: two bf16 roundings of 2^-8).
    bound: of the fp32 value.  -> max(err / bound) of hi + lo."""
    if kind == "split3":
        hi, hi2, lo = decode_split3(img, n)
        if not torch.equal(hi, hi2):
            raise AssertionError("%s: the two hi planes differ" % tag)
    else:
        hi, lo = decode_hl(img, n)
    if not torch.equal(hi, f32_run.to(torch.bfloat16)):
        at = (hi.view(torch.int16) != f32_run.to(torch.bfloat16).view(torch.int16)).nonzero()[0].tolist()
        raise AssertionError("%s: hi plane is not bf16 of the fp32 output, first at %s" % (tag, at))
    check(tag + " hi", hi, ref, bound + 2.0 ** -8 * ref.abs(), gate_hi)
    return check(tag + " hi+lo", hi.double() + lo.double(), ref, bound + 2.0 ** -16 * ref.abs(), gate_sum)


def moments64(x, group=32):
    """(sum, sum of squares, sum of magnitudes, sum of squares again as its own magnitude) per `group` columns of x, fp64."""
    v = x.double().reshape(x.shape[0], x.shape[1] // group, group)
    return v.sum(-1), (v * v).sum(-1), v.abs().sum(-1)


def check_moments(tag, part, x):
    """EPI 2: the (sum, sum of squares) pairs [m, n / 32, 2] against the fp64 sums of the new x the kernel wrote: 32 additions each."""
    s1, s2, sa = moments64(x)
    eps = 32 * 2.0 ** -23
    e1, e2 = (part[..., 0].double() - s1).abs(), (part[..., 1].double() - s2).abs()
    if not bool(torch.isfinite(part).all()) or bool((e1 > eps * sa).any()) or bool((e2 > eps * s2).any()):
        raise AssertionError("%s: moments off: sum %.3e of %.3e, squares %.3e of %.3e" % (
            tag, float(e1.max()), float((eps * sa).min()), float(e2.max()), float((eps * s2).min())))
    return max(float((e1 / (eps * sa).clamp_min(1e-300)).max()), float((e2 / (eps * s2).clamp_min(1e-300)).max()))


_recorded = collections.OrderedDict()


def record(entry, out, act, state, ratio):
    """max(err / bound) per (entry, output, act, state); printed by the GPU file as it goes."""
    key = (entry, out, act, state)
    _recorded[key] = max(_recorded.get(key, 0.0), ratio)
    return _recorded[key]
