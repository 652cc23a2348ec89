"""The native head widths of the inference attention (tests/attn_widths.py: fp32-class 192 and 256, bf16 256, bf16 192 packed), the part
that needs no GPU: the plan and workspace entry points of each width (pure host code; cu_count() falls back to the MI355X's 256 without
a device), the predicates and switches behind ``functional.encoder_layer`` / ``packed.pack_groups``, and the scratch bytes / registers
of the kernels.  The recipes are the reference README's: MAE (D = 768, h = 4, Lambda = 500) at 192, SimCLR ResNet-18 (D = 512, h = 2,
Lambda = 900 as 200 + 700) at 256."""
import ctypes

import numpy as np

from snuffy_amd import _ffi
from tests.attn_widths import (MFMA_256, MFMA_SCRATCH, STATS_SCRATCH, VARLEN_192, VL_DESC, X3_192, X3_256, _nkb, _offsets, _plan, _r256,
                               built_kernels, rows)

PLANNED = (X3_192, X3_256, MFMA_256, VARLEN_192)
OLDER_PLANS = {"x3": ("snf_sparse_attn_x3_varlen_plan", "snf_sparse_attn_x3_varlen_chunked_plan"),
               "mfma": ("snf_sparse_attn_varlen_plan", "snf_sparse_attn_varlen_chunked_plan")}


@rows(*PLANNED)
def test_every_key_count_has_built_chunks(row):
    """The chunk rule, for EVERY k: ceil(k / 128) chunks, at most 8, of ceil(k / chunks) keys (the fp32-class widths round that up to a
    multiple of 4), the last chunk shorter.  The plan reports it, the chunks cover k, and every chunk of a chunked launch needs a
    key-block count the MODE 1 / MODE 2 (192 packed: the chunked varlen) kernels are instantiated for.  Where the single-bag plan takes
    the same chunks (the 256 widths), its workspace follows: bf16 holds at least partial tiles + statistics."""
    lib = _ffi.load()
    seen = set()
    n, h = 300, 2
    for k in range(1, row.MAX_CHUNKS * row.KMAX + 1):
        rc, _, ws_v, nc, ck = _plan(row, lib, [n, 5000], k, h, table=False)
        assert rc == 0, k
        assert nc == -(-k // row.KMAX), k
        if row is MFMA_256:
            assert nc <= row.MAX_CHUNKS, k
        assert 1 <= ck <= row.KMAX and (nc - 1) * ck < k <= nc * ck, (k, nc, ck)
        if row.CHUNK_MULTIPLE == 1:
            assert ck == -(-k // nc), (k, nc, ck)                               # make_chunks' rule
        if row is X3_256:
            assert getattr(lib, row.ws_fn)(n, k, h) > 0, k                      # the single-bag plan takes the same chunks
        if row is MFMA_256:
            ws1 = getattr(lib, row.ws_fn)(n, k, h)
            tiles = -(-n // row.ROWS) * h                                       # 20 tiles < 256 CUs: one per workgroup, two segments each
            assert ws1 >= tiles * 2 * _nkb(ck) * row.NCB * 4096 + (nc * h * n * 8 if nc > 1 else 0), k
            assert ws_v > 0
        if nc == 1:
            assert ck == k
            if row is not VARLEN_192:
                continue
        elif row.CHUNK_MULTIPLE == 4:
            assert ck % 4 == 0, (k, ck)
        for c in range(nc):
            kc = min(ck, k - c * ck)
            assert 1 <= kc <= row.KMAX, (k, c)
            if nc > 1:
                seen.add(_nkb(kc))
    assert seen == {2, 4}, seen                                                # the counts the *_chunks.hip files build


@rows(*PLANNED)
def test_refusals(row):
    lib = _ffi.load()
    h, dk, top = row.H_PLAN, row.dk, row.MAX_CHUNKS * row.KMAX
    plan = getattr(lib, row.plan_fn)
    assert _plan(row, lib, [1000, 2000], top + 1, h)[0] == _ffi.SNF_EUNSUPPORTED
    assert b"unsupported" in lib.snf_last_error()
    if row is not VARLEN_192:
        assert _plan(row, lib, [1000, 2000], 0, h)[0] == _ffi.SNF_EUNSUPPORTED
        if row is not X3_192:
            assert b"unsupported" in lib.snf_last_error()
    if row is MFMA_256:
        assert _plan(row, lib, [1000, 2000], 900, 0)[0] == _ffi.SNF_EUNSUPPORTED
        assert b"unsupported" in lib.snf_last_error()
    assert _plan(row, lib, [1000, 2000], top, h)[0] == 0
    off = np.array([0, 100, 100], dtype=np.int64)                             # an empty bag (n = 0)
    need = ctypes.c_size_t(0)
    assert plan(ctypes.c_void_p(off.ctypes.data), 2, 300, h, None, 0, ctypes.byref(need), None, None, None) == _ffi.SNF_EUNSUPPORTED
    assert b"unsupported" in lib.snf_last_error()
    o2 = _offsets([1000, 2000])
    ws = ctypes.c_size_t(0)
    if row is MFMA_256:
        # a table that is too short
        assert plan(ctypes.c_void_p(o2.ctypes.data), 2, 300, 2, None, 0, ctypes.byref(need), ctypes.byref(ws), None, None) == 0
        short = np.zeros(need.value - 1, dtype=np.int32)
        assert plan(ctypes.c_void_p(o2.ctypes.data), 2, 300, 2, ctypes.c_void_p(short.ctypes.data), short.size, ctypes.byref(need),
                    ctypes.byref(ws), None, None) == _ffi.SNF_EUNSUPPORTED
        assert b"unsupported" in lib.snf_last_error() and b"table" in lib.snf_last_error()
        assert not short.any()                                                # nothing written
        # the single-bag workspace: 0 = unsupported
        for n, k, h_ in ((3000, 0, 2), (3000, 1025, 2), (3000, 900, 0), (0, 900, 2), (0xffff01, 100, 2)):
            assert lib.snf_sparse_attn_fwd_mfma_dk256_workspace_bytes(n, k, h_) == 0, (n, k, h_)
        assert lib.snf_sparse_attn_fwd_mfma_dk256_workspace_bytes(0xffff00, 100, 2) > 0
    # the older plan / workspace functions (64 / 128 / chunked) keep refusing the width: those of the row's own family, and at bf16 256
    # the fp32-class ones too
    for fam in (("mfma", "x3") if row is MFMA_256 else (row.family,)):
        plain, chunked = (getattr(lib, name) for name in OLDER_PLANS[fam])
        assert plain(ctypes.c_void_p(o2.ctypes.data), 2, 100, h, dk, None, 0, ctypes.byref(need), ctypes.byref(ws)) == _ffi.SNF_EUNSUPPORTED
        assert chunked(ctypes.c_void_p(o2.ctypes.data), 2, row.LAM, h, dk, None, 0, ctypes.byref(need), ctypes.byref(ws), None,
                       None) == _ffi.SNF_EUNSUPPORTED
    if row is not VARLEN_192:                                                 # the single bag of bf16 192 is the older function's
        for k in (100, row.LAM):
            assert lib.snf_sparse_attn_fwd_x3_workspace_bytes(4096, k, h, dk) == 0
            if row is MFMA_256:
                assert lib.snf_sparse_attn_fwd_workspace_bytes(4096, k, h, dk, 1) == 0
    if row is X3_256:
        # the entry points of 192 take no width: a dk = 256 operand does not fit their row pitch of h * 192, and their answers for
        # (n, k, h) are the pinned ones (tests/golden/attn_plans.npz) -- what they must not do is follow the new family's geometry
        n, k, h = 3000, 900, 2
        w192 = lib.snf_sparse_attn_fwd_x3_dk192_workspace_bytes(n, k, h)
        assert w192 == -(-n // 64) * h * 2 * 4 * 6 * 4096 + 8 * h * n * 8     # 64-row tiles, 6 column blocks: its own closed form
        assert w192 != lib.snf_sparse_attn_fwd_x3_dk256_workspace_bytes(n, k, h)
    if row is MFMA_256:
        # the fp32-class kernel of this width answers exactly as before: 32-row tiles, one (max, sum) pair per chunk, head and row, no
        # staging
        for n, k, h in ((3000, 900, 2), (300, 100, 2), (5000, 129, 1)):
            tiles, chunks = -(-n // X3_256.ROWS) * h, -(-k // X3_256.KMAX)
            size = k if chunks == 1 else (-(-k // chunks) + 3) & ~3
            assert lib.snf_sparse_attn_fwd_x3_dk256_workspace_bytes(n, k, h) == (tiles * 2 * _nkb(size) * X3_256.NCB * 4096
                                                                                + (chunks * h * n * 8 if chunks > 1 else 0)), (n, k, h)


@rows(X3_192, X3_256, MFMA_256)
def test_single_bag_workspace_follows_the_predicate(row):
    from snuffy_amd import ops
    lib = _ffi.load()
    ws, h = getattr(lib, row.ws_fn), row.H_PLAN
    for k in (-1, 0, 1, 20, 128, 129, row.LAM, 1024, 1025, 4096):
        assert (ws(3000, k, h) > 0) == getattr(ops, row.single_supported)(k), k
    if row.family == "x3":
        assert ws(0, 100, h) == 0
        assert ws(3000, 100, 0) == 0
    # chunked: partial tiles at the largest chunk's 4 key blocks | one (max, sum) pair per chunk, head and row | at bf16, the bf16 copy
    # of an f32 Kp (rounded to 256 bytes)
    n, k = 3000, row.LAM
    tiles = -(-n // row.ROWS) * h                                              # 188 < 256 CUs: one tile per workgroup, two segments
    chunks = -(-k // row.KMAX)                                                 # 192: 4 chunks; 256: 8 (116 / 113 keys): 4 key blocks
    staging = _r256(k * h * row.dk * 2) if row.family == "mfma" else 0
    assert ws(n, k, h) == tiles * 2 * 4 * row.NCB * 4096 + chunks * h * n * 8 + staging


@rows(*PLANNED)
def test_plan_geometry(row):
    lib = _ffi.load()
    sizes, k, h = [1000, 2000], 129, row.H_PLAN                                # 68 + 61 keys (bf16: 65 + 64): 4 and 2 key blocks
    rc, table, ws, nc, ck = _plan(row, lib, sizes, k, h)
    assert rc == 0 and (nc, ck) == (2, row.CK_129)
    b = len(sizes)
    desc = table[:VL_DESC * b].reshape(b, VL_DESC)
    off = _offsets(sizes)
    for i, n in enumerate(sizes):
        assert desc[i][1] == off[i] and desc[i][2] == n
        assert desc[i][3] == i * k                                            # first Kp / output row: the FULL key count
        if row in (X3_256, MFMA_256):
            assert desc[i][4] == -(-n // row.ROWS)                            # 32-row tiles
    slots = int(sum(int(d[9]) * int(d[7]) for d in desc))
    total = sum(sizes)
    tiles, stats = slots * _nkb(ck) * row.NCB * 4096, nc * h * total * 8
    if row is X3_256:
        assert ws == tiles + stats
    elif row is MFMA_256:
        assert ws == _r256(tiles) + _r256(stats) + _r256(k * b * h * row.dk * 2)
    else:
        assert ws >= tiles + stats
    # the geometry is the one-chunk plan's at the chunk size: it depends on n and h only
    rc1, t1, ws1, nc1, ck1 = _plan(row, lib, sizes, ck, h)
    assert rc1 == 0 and (nc1, ck1) == (1, ck)
    d1 = t1[:VL_DESC * b].reshape(b, VL_DESC)
    assert np.array_equal(np.delete(d1, 3, axis=1), np.delete(desc, 3, axis=1)) and np.array_equal(t1[VL_DESC * b:], table[VL_DESC * b:])
    assert [int(d[3]) for d in d1] == [0, ck]
    # one chunk: no statistics area -- partial tiles (+ at bf16 the staging of an f32 Kp, 2 bytes per element rounded up to 256)
    assert ws1 == _r256(tiles) + (_r256(ck * b * h * row.dk * 2) if row.family == "mfma" else 0)
    if row is not VARLEN_192:
        # the recipe: MAE 4 chunks of 128, 128, 128, 116 keys; SimCLR 8 chunks of ceil(900 / 8) = 113 (-> 116 fp32-class) keys
        assert _plan(row, lib, sizes, row.LAM, h, table=False)[3:] == row.RECIPE_CHUNKS
    # a bag of at most 1024 rows is one workgroup per head (stored directly), a longer one is reduced
    rc, table, _, _, _ = _plan(row, lib, [1024, 1025], 100, h)
    desc = table[:VL_DESC * 2].reshape(2, VL_DESC)
    assert rc == 0 and [int(d[10]) for d in desc] == [1, 0] and int(desc[0][9]) == h


@rows(*PLANNED)
def test_predicates_and_switches(row, monkeypatch):
    from snuffy_amd import functional as SF
    from snuffy_amd import ops, packed
    dk, kind, D, H, K = row.dk, row.kind, row.D, row.H, row.LAM
    if row is not VARLEN_192:
        assert [getattr(ops, row.single_supported)(k) for k in row.PRED_KS] == row.PRED_WANT
    assert [getattr(ops, row.varlen_supported)(k) for k in row.PRED_KS] == row.PRED_WANT
    if row is MFMA_256:
        # the 32-bit element offsets of the family: rows, row pitch, rows x pitch
        assert ops.mfma_attn_dk256_supported(900, 0xffff00, 128) and not ops.mfma_attn_dk256_supported(900, 0xffff01, 128)
        assert ops.mfma_attn_dk256_supported(900, 100, (1 << 24) - 8) and not ops.mfma_attn_dk256_supported(900, 100, 1 << 24)
        assert ops.mfma_attn_dk256_supported(900, 2097151, 1024) and not ops.mfma_attn_dk256_supported(900, 2097152, 1024)
    # the older predicates keep their answers at this width
    for older in (("bf16", "fp32") if row is VARLEN_192 else (kind,)):
        for k in (1, 128, 200, K):
            assert not ops.varlen_attn_supported(older, k, dk)
            assert not ops.varlen_attn_chunks_supported(older, k, dk)
            if row.family == "x3":
                assert not ops.x3_attn_supported(k, dk)
            if row is X3_256:
                assert ops.x3u_attn_supported(k, dk)
            if row is MFMA_256:
                assert not ops.mfma_attn_supported(k, dk)
    if row.dk == 256:
        assert SF.head_pad(256) is None and SF.packed_head_pad(256) is None
    if row is VARLEN_192:
        assert SF.packed_head_pad(192) is None
        assert isinstance(packed.PACK_DK192, bool)
    if row.family == "x3":
        # 192: both switches ship off; 256, the verdicts of profiles/x3_dk256.txt: the single bag stays on the unfused pair, packed bags
        # take the new kernel
        assert getattr(SF, row.single_switch) is row.SHIPPED[0] and getattr(packed, row.pack_switch) is row.SHIPPED[1]
    ok = getattr(packed, row.pack_ok)
    other = "fp32" if kind == "bf16" else "bf16"
    for on in (True, False):
        monkeypatch.setattr(packed, row.pack_switch, on)
        assert ok(kind, D, H, K) is on                                            # the recipe
        assert all(ok(kind, d, h, k) is on for d, h, k in row.OK_SHAPES)
        assert ok(kind, D, H, 1025) is False and ok(kind, D, H, 0) is False
        assert ok(kind, D, row.H_OTHER, K) is False                               # dk = 128: not this predicate's
        assert ok(other, D, H, K) is False                                        # the other precision has a predicate of its own, or none
        if row is X3_192:
            assert packed.dk192_ok("fp32", 768, 4, 500) is False                  # the bf16 predicate keeps refusing fp32
        if row is X3_256:
            assert packed.x3_dk192_ok("fp32", 512, 2, 900) is False and packed.dk192_ok("bf16", 512, 2, 900) is False
        if row is MFMA_256:
            assert packed.dk192_ok("bf16", 512, 2, 900) is False
            # fp32 is routed by its own switch, whatever this one says; neither consults the single-bag switch
            for x3_on in (True, False):
                monkeypatch.setattr(packed, "PACK_X3_DK256", x3_on)
                assert packed.x3_dk256_ok("fp32", 512, 2, 900) is x3_on and packed.x3_dk256_ok("bf16", 512, 2, 900) is False
        if row is VARLEN_192:
            for any_kind in ("bf16", "fp32"):                                     # PACK_KEY_CHUNKS does not take the width either way
                assert not packed.key_chunks_ok([], any_kind, 768, 4, 500, 5, 9000)
        else:
            # the single-bag switch is not consulted
            monkeypatch.setattr(SF, row.single_switch, not on)
            assert ok(kind, D, H, K) is on


@rows(X3_192, X3_256, MFMA_256)
def test_new_kernels_keep_their_scratch(row):
    """Scratch bytes per lane of <kernel><NKB, AUX, MODE, VL> against the row's table; at bf16 256 the table holds (VGPRs, scratch),
    nothing spills and the single-bag forms have zero scratch."""
    got, reduced = {}, set()
    for (obj, _, scratch, spilled, vgpr), name, args in built_kernels(row.obj + ".o"):
        if row.kernel in name:
            assert obj == (row.obj + ".o" if args[2] == "0" else row.obj + "_chunks.o"), (obj, name)
            if row is MFMA_256:
                assert spilled == 0, name
            got[(int(args[0]), args[1] == "true", int(args[2]), args[3] == "true")] = (vgpr, scratch) if row is MFMA_256 else scratch
        elif row.reduce in name and (row is not MFMA_256 or obj.startswith(row.obj)):
            assert scratch == 0, name
            reduced.add(int(args[1]))
        assert not any(old in name for old in row.absent), name
    if row is MFMA_256:
        assert all(s == 0 for (_, _, _, vl), (_, s) in got.items() if not vl)  # the condition: single-bag forms have zero scratch
    assert got == row.TABLE
    assert reduced == {1, 2, 4}


@rows(VARLEN_192)
def test_packed_192_kernels_keep_their_scratch(row):
    mfma, stats, old = {}, {}, {"fwd": 0, "stats": 0, "bwd": 0}
    for (obj, _, scratch, _, _), name, args in built_kernels("sparse_attn_mfma_varlen_dk192.o"):
        if "sparse_attn_mfma_vl192_kernel<" in name:
            assert obj == "sparse_attn_mfma_varlen_dk192.o", (obj, name)
            assert args[0] == "192" and args[2] == "unsigned short" and args[5] == "8" and args[6] == "true", name
            mfma[(int(args[1]), args[3] == "true", args[4] == "true")] = scratch
        elif "sparse_attn_stats_vl192_kernel<" in name:
            assert obj == "sparse_attn_mfma_varlen_dk192.o", (obj, name)
            assert args[0] == "192" and args[2] == "unsigned short" and args[3] == "true", name
            stats[int(args[1])] = scratch
        old["fwd"] += "sparse_attn_mfma_kernel<192," in name
        old["stats"] += "sparse_attn_stats_kernel<192," in name
        old["bwd"] += "sparse_attn_bwd_chunk_kernel<192," in name
    assert mfma == MFMA_SCRATCH
    assert stats == STATS_SCRATCH
    assert old == {"fwd": 20, "stats": 4, "bwd": 5}, old                          # the single-bag kernels of the width keep their names
