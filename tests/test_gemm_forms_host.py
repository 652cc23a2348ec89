"""The form table of tests/gemm_forms.py is complete and its checkers are sharp, without a device: every entry meets every K-step state on
an edge shape and every walk state on a walk shape, the restated walk gives the pinned row counts at 256 CUs, the restated split geometry is
the library's, the domain limits are the library's, and every corruption the suite is there for is flagged by the same check_* functions the
GPU file uses.  (Without a device the library sizes its grids for 256 compute units.)"""
import ctypes

import numpy as np
import pytest
import torch

from tests import gemm_forms as GF

CUS = 256
NBUF, AHEAD = 4, 2


# ---- completeness ----------------------------------------------------------------------------------------------------------------------------
def test_the_table_names_every_launched_family():
    assert list(GF.ENTRIES) == ["gemm_bf16", "gemm_bf16_resid_f32", "gemm_x3_resid_f32", "gemm_bf16_dropout", "gemm_bf16_lnfold",
                                "gemm_bf16_resid_", "gemm_hl", "gemm_hl_split", "gemm_hl_dropout", "gemm_hl_deferred", "gemm_hl_gated",
                                "linear_rows_x3", "linear_rows_x3_resid"]
    assert {e.name: e.min_k for e in GF.ENTRIES.values()} == {
        "gemm_bf16": 64, "gemm_bf16_resid_f32": 64, "gemm_x3_resid_f32": 64, "gemm_bf16_dropout": 64, "gemm_bf16_lnfold": 96,
        "gemm_bf16_resid_": 96, "gemm_hl": 32, "gemm_hl_split": 512, "gemm_hl_dropout": 32, "gemm_hl_deferred": 512, "gemm_hl_gated": 32,
        "linear_rows_x3": 16, "linear_rows_x3_resid": 16}


def test_the_k_step_states_are_what_their_names_say():
    assert [k // 32 for k in GF.K_BF16] == [AHEAD, AHEAD + 1, NBUF, NBUF + 1, 9] and 9 % NBUF != 0
    assert GF.K_EPI == GF.K_BF16[1:] and [k // 32 for k in GF.K_HL] == [1, 2, 3, 5]
    steps = [k // 16 for k in GF.K_SKINNY]
    per = [-(-s // 8) for s in steps]
    assert steps[:3] == [1, 2, 3] and all(s < 8 for s in steps[:3])                 # fewer steps than waves
    assert steps[3] == 9 and per[3] == 2 and 9 % 2                                  # an uneven share: the fifth wave gets one step
    assert steps[4] == 50 and per[4] == 7                                           # a second batch of 6 holding one live step
    assert steps[5] == 48 and per[5] == 6                                           # exactly one batch


@pytest.mark.parametrize("name", GF.TILE_ENTRIES)
def test_every_entry_meets_every_k_step_state_on_every_edge_shape(name):
    e = GF.ENTRIES[name]
    cases = GF.edge_cases(e)
    assert min(e.ks) == e.min_k or e.operands == "x3"                               # (x3 images: three times the true k, 96 and 288 columns)
    for w in e.widths:
        for o in e.outs:
            for a in GF.out_acts(e, o):
                got = {(m, n, k) for cw, co, ca, m, n, k in cases if (cw, co, ca) == (w, o, a)}
                assert got == {(m, n, k) for m, n in GF.edge_shapes(e, o) for k in e.ks}, (name, w, o, a)
            assert all(n % GF.out_gran(e, o) == 0 for _, n in GF.edge_shapes(e, o))
    assert set(a for _, _, a, _, _, _ in cases) == set(e.acts)


@pytest.mark.parametrize("shapes", [GF.EDGE, GF.EDGE_32, GF.EDGE_64])
@pytest.mark.parametrize("bn", [256, 128])
def test_edge_shapes_are_one_tile_per_workgroup_ragged_both_ways(shapes, bn):
    rows_cut = cols_cut = both_cut = full = False
    for m, n in shapes:
        st = GF.walk_states(m, n, bn, CUS)
        assert st.lengths == {1} and not st.transitions
        tn = -(-n // bn)
        for seq in GF.walk(m, n, bn, CUS).values():
            (t, f), = seq
            r, c = (t // tn + 1) * 256 > m, (t % tn + 1) * bn > n
            assert f == (not r and not c)
            rows_cut, cols_cut, both_cut, full = rows_cut or (r and not c), cols_cut or (c and not r), both_cut or (r and c), full or f
    assert rows_cut and cols_cut and both_cut and full
    assert (512, 512) in shapes and GF.walk_states(512, 512, bn, CUS).first == {"F"}


@pytest.mark.parametrize("name", GF.TILE_ENTRIES)
def test_every_form_and_store_class_meets_both_walk_shapes(name):
    e = GF.ENTRIES[name]
    cases = GF.walk_cases(e, CUS)
    widths = (256, 128) if name == "gemm_bf16_resid_" else e.widths
    for w in widths:
        for o in e.outs:
            classes = {GF.store_class(a) for a in GF.out_acts(e, o)}
            for cl in classes:
                lengths = {L for cw, co, ca, L, m, n, k in cases if (cw, co) == (w, o) and GF.store_class(ca) == cl}
                assert lengths == set(GF.WALK_LENGTHS), (name, w, o, cl)
    for w, o, a, L, m, n, k in cases:
        assert k in GF.walk_ks(e) and n % GF.out_gran(e, o) == 0 and m % 256 == 37
        st = GF.walk_states(m, n, w or 256, CUS)
        assert st.transitions == {"FF", "FP", "PF", "PP"} and st.lengths == {L - 1, L}, (name, w, m, n, st)
        assert m * (k * (3 if e.operands != "bf16" else 1) + GF.PAD) < 2 ** 31        # 31-bit element offsets of the pitched operand


def test_walk_rows_at_256_cus_are_pinned():
    """Three ragged 256-wide column tiles (n = 576, 704) / five ragged 128-wide ones (n = 576): the walk depends on the tile counts alone."""
    assert [GF.walk_rows(576, 256, CUS, L) for L in (2, 3)] == [23077, 43557]
    assert [GF.walk_rows(704, 256, CUS, L) for L in (2, 3)] == [23077, 43557]
    assert [GF.walk_rows(576, 128, CUS, L) for L in (2, 3)] == [14629, 26149]
    def reaches(m, n, bn, length):
        st = GF.walk_states(m, n, bn, CUS)
        return st.transitions == {"FF", "FP", "PF", "PP"} and st.lengths == {length - 1, length}

    for n, bn, m, length in ((576, 256, 23077, 2), (704, 256, 43557, 3), (576, 128, 14629, 2), (576, 128, 26149, 3)):
        st = GF.walk_states(m, n, bn, CUS)
        assert reaches(m, n, bn, length) and st.first == {"F", "P"} and st.last == {"F", "P"}
        assert not any(reaches(256 * t + 37, n, bn, length) for t in range(m // 256))    # the smallest
    assert -(-576 // 256) == 3 and -(-704 // 256) == 3 and -(-576 // 128) == 5 and 576 % 64 == 0 and 704 % 256 > 128 and 1 <= 576 % 256 <= 128


def test_the_walk_covers_every_tile_once():
    for m, n, bn in ((43557, 704, 256), (26149, 576, 128), (300, 264, 128), (1, 136, 256), (22400, 768, 256)):
        tiles = sorted(t for seq in GF.walk(m, n, bn, CUS).values() for t, _ in seq)
        assert tiles == list(range(-(-m // 256) * -(-n // bn)))
        assert all(b % 8 == x for b, seq in GF.walk(m, n, bn, CUS).items() for x in [b & 7] for t, _ in seq
                   if GF.xcd_range(len(tiles), x)[0] <= t < GF.xcd_range(len(tiles), x)[1])


# ---- the split geometry ------------------------------------------------------------------------------------------------------------------------
def test_split_geometry_is_the_librarys():
    for m0, n, _ in GF.SPLIT_SHAPES:
        for m in range(max(1, m0 - 2560), m0 + 2561, 256):
            for k in (480, 512, 544, 800, 1024):
                g = GF.split_geometry(m, n, k, CUS)
                assert g.ws_bytes == GF.lib_ws_bytes(m, n, k), (m, n, k)
                nbytes, off = GF.lib_deferred_bytes(m, n, k)
                assert g.deferred_bytes == nbytes and (not nbytes or g.slab_offset == off), (m, n, k)
                assert bool(g.ws_bytes) == bool(g.tiles) == bool(nbytes)


def test_the_split_shapes_have_the_stated_parts():
    g = GF.split_geometry(900, 768, 544, CUS)                     # 12 tiles on 16 workgroups: XCDs 4 - 7 split in 2, 17 steps -> 8 + 9
    assert GF.grid_of(12, CUS) == 16 and [p for _, _, p in g.xcds] == [1, 1, 1, 1, 2, 2, 2, 2] and GF.part_steps(17, 2) == [8, 9]
    assert sorted(g.tiles) == [8, 9, 10, 11] and 3 * 256 < 900 < 4 * 256          # tiles 9 - 11 are the ragged last row panel
    g = GF.split_geometry(22400, 768, 800, CUS)                   # 264 tiles: r = 1 on every XCD, 3 parts of 8, 8, 9 steps
    assert all((q, r, p) == (33, 1, 3) for q, r, p in g.xcds) and GF.part_steps(25, 3) == [8, 8, 9]
    assert max(g.tiles) == 263 and 22400 % 256                                     # the chip's last tile is split and partial
    g = GF.split_geometry(22400, 768, 1024, CUS)
    assert all(p == 4 for _, _, p in g.xcds) and GF.part_steps(32, 4) == [8, 8, 8, 8]
    g = GF.split_geometry(900, 768, 480, CUS)                     # 15 steps: below two parts of HL_SPLIT_MIN_STEPS
    assert not g.tiles and g.ws_bytes == 0 and [r for _, r, _ in g.xcds] == [0, 0, 0, 0, 1, 1, 1, 1]
    g = GF.split_geometry(33000, 520, 1024, CUS)                  # mixed: XCDs 0 - 2 (r = 17 of 32) do not split, 3 - 7 (r = 16) do
    assert [p for _, _, p in g.xcds] == [1, 1, 1, 2, 2, 2, 2, 2] and g.rcap == 16 and len(g.tiles) == 80
    for m, n, k in GF.SPLIT_SHAPES:
        assert k >= 512 or not GF.split_geometry(m, n, k, CUS).tiles


# ---- domain --------------------------------------------------------------------------------------------------------------------------------------
def test_the_wrappers_domain_rules_agree_with_the_table():
    from snuffy_amd import ops
    e = GF.ENTRIES
    assert ops.gemm_supported(1, 8, e["gemm_bf16"].min_k) and not ops.gemm_supported(1, 8, e["gemm_bf16"].min_k - 32)
    assert not ops.gemm_supported(1, 12, 64) and not ops.gemm_supported(1, 8, 80)
    assert ops.gemm_lnfold_supported(64, e["gemm_bf16_lnfold"].min_k) and not ops.gemm_lnfold_supported(64, 64)
    assert not ops.gemm_lnfold_supported(32, 96) and e["gemm_bf16_resid_"].gran == e["gemm_bf16_lnfold"].gran == 64
    assert ops.hl_eligible(10 ** 5, 256, e["gemm_hl"].min_k) and not ops.hl_eligible(10 ** 5, 256, 16) and not ops.hl_eligible(10 ** 5, 260, 32)
    assert ops.linear_rows_x3_supported(1, 1, 16) and not ops.linear_rows_x3_supported(1, 1, 8) and not ops.linear_rows_x3_supported(1, 1, 24)
    assert ops.linear_rows_x3_supported(8192, 1, 16) and not ops.linear_rows_x3_supported(8193, 1, 16)


def test_one_step_below_each_minimum_is_refused_before_any_launch():
    """The C entries check their arguments before they touch a device: valid host addresses, a k one step short, a non-zero return."""
    from snuffy_amd import _ffi
    lib = GF.lib()
    buf = np.zeros(1 << 16, dtype=np.uint8)
    p = ctypes.c_void_p((buf.ctypes.data + 255) & ~255)
    refused = (_ffi.SNF_EINVAL, _ffi.SNF_EUNSUPPORTED)
    m, n = 64, 64
    assert lib.snf_gemm_bf16(p, 128, p, 128, p, m, n, 32, 4, p, 128, 0, 0, None) in refused
    assert b"k >= 64" in lib.snf_last_error()
    assert lib.snf_gemm_bf16_resid_f32(p, 128, p, 128, p, p, 128, m, n, 32, 4, p, 128, 0, None) in refused
    assert lib.snf_gemm_bf16_dropout(p, 128, p, 128, p, m, n, 32, 0, p, 128, 1, 0, 0.5, 1, 0, None) in refused
    assert lib.snf_gemm_bf16_lnfold(p, 128, p, 128, p, p, p, m, n, 64, 4, p, 128, None) in refused
    assert b"k >= 96" in lib.snf_last_error()
    assert lib.snf_gemm_bf16_resid(p, 128, p, 128, p, m, n, 64, p, 128, p, 128, p, None) in refused
    for k in (0, 16):
        assert lib.snf_gemm_hl_ws_bf16(p, 128, p, 128, p, None, 0, m, n, k, 4, p, 128, 0, None, 0, None) in refused
        assert lib.snf_gemm_hl_gated_bf16(p, 128, p, 128, p, 128, m, n, k, p, 128, None) in refused
        assert lib.snf_gemm_hl_ws_dropout_bf16(p, 128, p, 128, p, None, 0, m, n, k, 4, p, 128, 0, 0.5, 1, 0, None, 0, None) in refused
    assert lib.snf_gemm_hl_ws_bytes(900, 768, 480) == 0 and lib.snf_gemm_hl_ws_bytes(900, 768, 512) > 0
    assert lib.snf_gemm_hl_deferred_f32(p, 1024, p, 1024, p, None, 0, 900, 768, 480, 4, p, 768, 0, p, 1 << 15, None) == _ffi.SNF_EUNSUPPORTED
    assert lib.snf_linear_rows_x3_f32(p, 64, p, 64, p, 1, 1, 8, p, 64, 0, None) in refused
    assert lib.snf_linear_rows_x3_resid_f32(p, 64, p, 64, p, p, 64, 1, 1, 8, p, 64, p, 64, None) in refused


# ---- the checker catches what it is for ------------------------------------------------------------------------------------------------------------
M, N, K = 600, 576, 1024                     # 3 x 3 tiles of 256 (ragged both ways) at the largest k of the table


@pytest.fixture(scope="module")
def cpu_case():
    op = GF.operands(M, N, K, bn=256, device="cpu")
    out = {}
    for cls in ("bf16", "fp32"):
        a, w = (op.a.to(torch.bfloat16).double(), op.w.to(torch.bfloat16).double()) if cls == "bf16" else (op.a.double(), op.w.double())
        out[cls] = (a, w, GF.contraction(a, w, op.bias))
    return op, out


def _tile(tm, tn):
    return slice(256 * tm, min(256 * (tm + 1), M)), slice(256 * tn, min(256 * (tn + 1), N))


def _flagged(got, ref, bound, gate=GF.GATE_X3_F32):
    with pytest.raises(AssertionError):
        GF.check("corrupted", got, ref, bound, gate)


@pytest.mark.parametrize("cls", ["bf16", "fp32"])
@pytest.mark.parametrize("act", GF.ACTS)
def test_the_reference_itself_passes_and_every_tile_fault_is_flagged(cpu_case, cls, act):
    op, per = cpu_case
    a, w, r = per[cls]
    gate = GF.GATE_BF16_F32 if cls == "bf16" else GF.GATE_X3_F32
    ref, bound = GF.expected(r, cls, K, act)
    assert GF.check("clean", ref.float(), ref, bound, gate) < 0.1                    # fp32 rounding of the exact result: far inside
    rs, cs = _tile(1, 1)

    def through(p):
        return GF.ref_act(p, act).float()
    # one 16 x 8 fragment taken from the neighbouring wave's position (128 rows / 64 columns further)
    for dr, dc in ((128, 0), (0, 64)):
        p = r.p.clone()
        p[256:272, 256:264] = r.p[256 + dr:272 + dr, 256 + dc:264 + dc]
        _flagged(through(p), ref, bound, gate)
    # one 32-column step missing from one tile
    p = r.p.clone()
    p[rs, cs] -= a[rs, 32:64] @ w[cs, 32:64].t()
    got = through(p)
    _flagged(got, ref, bound, gate)
    if act == "none":
        assert float(((got.double() - ref).abs() > bound)[rs, cs].double().mean()) > 0.5      # ... in most of the tile's elements
    # one step computed from the previous tile's A rows
    p = r.p.clone()
    p[rs, cs] += (a[0:256, 0:32] - a[rs, 0:32]) @ w[cs, 0:32].t()
    _flagged(through(p), ref, bound, gate)
    # the neighbouring column tile's bias
    p = r.p.clone()
    p[rs, cs] += (op.bias[0:256] - op.bias[cs]).double()
    _flagged(through(p), ref, bound, gate)
    # a NaN in one element
    got = ref.float().clone()
    got[M - 1, N - 1] = float("nan")
    _flagged(got, ref, bound, gate)


def test_a_small_wrong_value_where_relu_gave_zero_is_flagged(cpu_case):
    """... which the max-norm gate of a bf16 output passes."""
    _, per = cpu_case
    a, w, r = per["bf16"]
    ref, bound = GF.expected(r, "bf16", K, "relu", rounded=True)
    got = ref.to(torch.bfloat16)
    GF.check("clean", got, ref, bound, GF.GATE_BF16_OUT)
    at = tuple((ref == 0).nonzero()[7].tolist())
    got[at] = 1e-3 * float(ref.abs().max())
    err = (got.double() - ref).abs().max().item()
    assert err <= GF.GATE_BF16_OUT * max(1.0, float(ref.abs().max()))                # the old gate alone passes it
    _flagged(got, ref, bound, GF.GATE_BF16_OUT)


@pytest.mark.parametrize("kind", ["hl", "split3"])
def test_swapped_image_halves_are_flagged(cpu_case, kind):
    _, per = cpu_case
    a, w, r = per["fp32"]
    ref, bound = GF.expected(r, "fp32", K, "none")
    val = ref.float()
    img = GF.image_hl(val) if kind == "hl" else GF.image_x3(val)
    GF.check_image("clean", kind, img, N, val, ref, bound, GF.GATE_BF16_OUT, GF.GATE_X3_F32)
    bad = img.clone()
    if kind == "hl":
        bad[:, 64 * 3:64 * 3 + 32], bad[:, 64 * 3 + 32:64 * 4] = img[:, 64 * 3 + 32:64 * 4], img[:, 64 * 3:64 * 3 + 32]
    else:
        bad[:, 96:128], bad[:, 2 * N + 96:2 * N + 128] = img[:, 2 * N + 96:2 * N + 128], img[:, 96:128]
    with pytest.raises(AssertionError):
        GF.check_image("swapped", kind, bad, N, val, ref, bound, GF.GATE_BF16_OUT, GF.GATE_X3_F32)
    # a lo plane that is merely absent: hi alone is 2^-8 off, past the 2^-16 of hi + lo
    bad = img.clone()
    if kind == "hl":
        bad[:, 32:64] = 0
    else:
        bad[:, 2 * N:2 * N + 32] = 0
    with pytest.raises(AssertionError):
        GF.check_image("no lo", kind, bad, N, val, ref, bound, GF.GATE_BF16_OUT, GF.GATE_X3_F32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.int32])
@pytest.mark.parametrize("rows_only", [False, True])
def test_stores_past_the_matrix_are_flagged(dtype, rows_only):
    g = GF.Guarded(300, 264, dtype, device="cpu", rows_only=rows_only)
    assert g.view.shape == (300, 264) and (rows_only == g.view.is_contiguous())
    if dtype != torch.int32:
        assert bool(torch.isnan(g.view.float()).all())                                # an element the kernel never wrote is not finite
    g.view.zero_()
    g.intact()
    if not rows_only:
        g.view.as_strided((1, 272), (g.view.stride(0), 1))[0, 264:272] = 1            # one 8-column group written past n
        with pytest.raises(AssertionError):
            g.intact()
        g = GF.Guarded(300, 264, dtype, device="cpu")
    g.view.as_strided((301, 264), g.view.stride())[300, :8] = 1                       # one row written past m
    with pytest.raises(AssertionError):
        g.intact()


def test_wrong_moments_are_flagged(cpu_case):
    _, per = cpu_case
    x = per["bf16"][2].p.float()
    s1, s2, _ = GF.moments64(x)
    part = torch.stack((s1, s2), -1).float()
    assert GF.check_moments("clean", part, x) < 0.2
    bad = part.clone()
    bad[5, 3] = part[5, 4]                                                            # the neighbouring group's pair
    with pytest.raises(AssertionError):
        GF.check_moments("shifted", bad, x)
