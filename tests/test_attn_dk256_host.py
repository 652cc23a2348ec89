"""bf16 MFMA attention at head width 256 (the reference README's SimCLR ResNet-18 recipe: D = 512, h = 2, Lambda = 900 as 200 + 700, in
precision="bf16"), the part that needs no GPU: the workspace and plan entry points of the width (pure host code; cu_count() falls back to
the MI355X's 256 without a device), the predicates and switches behind ``functional.encoder_layer`` / ``packed.pack_groups``, and the
register / scratch table of the new kernels."""
import ctypes
import os
import sys

import numpy as np
import pytest

from snuffy_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

VL_DESC = 12
KMAX = 128                                                                      # keys per launch
MAX_CHUNKS = 8
ROWS = 32                                                                       # query rows per tile
NCB = 8                                                                         # 32-wide column blocks of a dk = 256 output tile row
DK = 256


def _offsets(sizes):
    off = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum(sizes, out=off[1:])
    return off


def _plan(lib, sizes, k, h, table=True):
    """(rc, table, workspace bytes, chunks, keys per chunk)"""
    fn, off = lib.snf_sparse_attn_varlen_dk256_plan, _offsets(sizes)
    need, ws, nc, ck = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = fn(ctypes.c_void_p(off.ctypes.data), len(sizes), k, h, None, 0, ctypes.byref(need), ctypes.byref(ws), ctypes.byref(nc),
            ctypes.byref(ck))
    if rc or not table:
        return rc, None, ws.value, nc.value, ck.value
    tab = np.full(need.value, -7, dtype=np.int32)
    assert fn(ctypes.c_void_p(off.ctypes.data), len(sizes), k, h, ctypes.c_void_p(tab.ctypes.data), tab.size, ctypes.byref(need),
              ctypes.byref(ws), None, None) == 0                              # the chunk outputs are nullable
    return 0, tab, ws.value, nc.value, ck.value


def _nkb(kc):
    """Key-block count the planner picks for a launch of kc keys."""
    return next(o for o in (1, 2, 4) if 32 * o >= kc)


def _r256(b):
    return -(-b // 256) * 256


def test_every_key_count_has_built_chunks():
    """The bf16 family's chunk rule at 128 keys per launch (ceil(k / 128) near-equal chunks of ceil(k / chunks) keys, the last one
    shorter), for EVERY k: at most 8 chunks, the plan reports the rule's sizes, the chunks cover k, every chunk of a chunked launch needs
    a key-block count the MODE 1 / MODE 2 kernels are instantiated for, and the workspace holds at least partial tiles + statistics."""
    lib = _ffi.load()
    seen = set()
    n, h = 300, 2
    for k in range(1, MAX_CHUNKS * KMAX + 1):
        rc, _, ws_v, nc, ck = _plan(lib, [n, 5000], k, h, table=False)
        assert rc == 0, k
        assert nc == -(-k // KMAX) <= MAX_CHUNKS, k
        assert ck == -(-k // nc), (k, nc, ck)                                   # make_chunks' rule
        assert 1 <= ck <= KMAX and (nc - 1) * ck < k <= nc * ck, (k, nc, ck)
        ws1 = lib.snf_sparse_attn_fwd_mfma_dk256_workspace_bytes(n, k, h)       # the single-bag plan takes the same chunks
        tiles = -(-n // ROWS) * h                                               # 20 tiles < 256 CUs: one per workgroup, two segments each
        assert ws1 >= tiles * 2 * _nkb(ck) * NCB * 4096 + (nc * h * n * 8 if nc > 1 else 0), k
        assert ws_v > 0
        if nc == 1:
            assert ck == k
            continue
        for c in range(nc):
            kc = min(ck, k - c * ck)
            assert 1 <= kc <= KMAX, (k, c)
            seen.add(_nkb(kc))
    assert seen == {2, 4}, seen                                                # the counts sparse_attn_mfma_dk256_chunks.hip builds


def test_refusals():
    lib = _ffi.load()
    for k, h in ((MAX_CHUNKS * KMAX + 1, 2), (0, 2), (900, 0)):
        assert _plan(lib, [1000, 2000], k, h)[0] == _ffi.SNF_EUNSUPPORTED, (k, h)
        assert b"unsupported" in lib.snf_last_error()
    assert _plan(lib, [1000, 2000], MAX_CHUNKS * KMAX, 2)[0] == 0
    off = np.array([0, 100, 100], dtype=np.int64)                             # an empty bag (n = 0)
    need = ctypes.c_size_t(0)
    assert lib.snf_sparse_attn_varlen_dk256_plan(ctypes.c_void_p(off.ctypes.data), 2, 300, 2, None, 0, ctypes.byref(need), None, None,
                                                 None) == _ffi.SNF_EUNSUPPORTED
    assert b"unsupported" in lib.snf_last_error()
    # a table that is too short
    o2 = _offsets([1000, 2000])
    ws = ctypes.c_size_t(0)
    assert lib.snf_sparse_attn_varlen_dk256_plan(ctypes.c_void_p(o2.ctypes.data), 2, 300, 2, None, 0, ctypes.byref(need), ctypes.byref(ws),
                                                 None, None) == 0
    short = np.zeros(need.value - 1, dtype=np.int32)
    assert lib.snf_sparse_attn_varlen_dk256_plan(ctypes.c_void_p(o2.ctypes.data), 2, 300, 2, ctypes.c_void_p(short.ctypes.data), short.size,
                                                 ctypes.byref(need), ctypes.byref(ws), None, None) == _ffi.SNF_EUNSUPPORTED
    assert b"unsupported" in lib.snf_last_error() and b"table" in lib.snf_last_error()
    assert not short.any()                                                    # nothing written
    # the single-bag workspace: 0 = unsupported
    for n, k, h in ((3000, 0, 2), (3000, 1025, 2), (3000, 900, 0), (0, 900, 2), (0xffff01, 100, 2)):
        assert lib.snf_sparse_attn_fwd_mfma_dk256_workspace_bytes(n, k, h) == 0, (n, k, h)
    assert lib.snf_sparse_attn_fwd_mfma_dk256_workspace_bytes(0xffff00, 100, 2) > 0
    # the older plan / workspace functions (64 / 128 / chunked, bf16 and fp32-class) keep refusing the width
    for fn in (lib.snf_sparse_attn_varlen_plan, lib.snf_sparse_attn_x3_varlen_plan):
        assert fn(ctypes.c_void_p(o2.ctypes.data), 2, 100, 2, 256, None, 0, ctypes.byref(need), ctypes.byref(ws)) == _ffi.SNF_EUNSUPPORTED
    for fn in (lib.snf_sparse_attn_varlen_chunked_plan, lib.snf_sparse_attn_x3_varlen_chunked_plan):
        assert fn(ctypes.c_void_p(o2.ctypes.data), 2, 900, 2, 256, None, 0, ctypes.byref(need), ctypes.byref(ws), None,
                  None) == _ffi.SNF_EUNSUPPORTED
    for k in (100, 900):
        assert lib.snf_sparse_attn_fwd_workspace_bytes(4096, k, 2, 256, 1) == 0
        assert lib.snf_sparse_attn_fwd_x3_workspace_bytes(4096, k, 2, 256) == 0
    # the fp32-class kernel of this width answers exactly as before: 32-row tiles, one (max, sum) pair per chunk, head and row, no staging
    for n, k, h in ((3000, 900, 2), (300, 100, 2), (5000, 129, 1)):
        tiles, chunks = -(-n // ROWS) * h, -(-k // KMAX)
        size = k if chunks == 1 else (-(-k // chunks) + 3) & ~3
        assert lib.snf_sparse_attn_fwd_x3_dk256_workspace_bytes(n, k, h) == (tiles * 2 * _nkb(size) * NCB * 4096
                                                                            + (chunks * h * n * 8 if chunks > 1 else 0)), (n, k, h)


def test_single_bag_workspace_follows_the_predicate():
    from snuffy_amd import ops
    lib = _ffi.load()
    for k in (-1, 0, 1, 20, 128, 129, 900, 1024, 1025, 4096):
        assert (lib.snf_sparse_attn_fwd_mfma_dk256_workspace_bytes(3000, k, 2) > 0) == ops.mfma_attn_dk256_supported(k), k
    # chunked: partial tiles at the largest chunk's 4 key blocks (rounded to 256 bytes) | one (max, sum) pair per chunk, head and row |
    # the bf16 copy of an f32 Kp (rounded to 256 bytes)
    n, k, h = 3000, 900, 2
    tiles = -(-n // ROWS) * h                                                  # 188 < 256 CUs: one tile per workgroup, two segments
    chunks = -(-k // KMAX)                                                     # 8 chunks of 113 keys (the last 109): 4 key blocks
    assert lib.snf_sparse_attn_fwd_mfma_dk256_workspace_bytes(n, k, h) == (tiles * 2 * 4 * NCB * 4096 + chunks * h * n * 8
                                                                           + _r256(k * h * DK * 2))


def test_plan_geometry():
    lib = _ffi.load()
    sizes, k, h = [1000, 2000], 129, 2                                         # 65 + 64 keys: 4 and 2 key blocks
    rc, table, ws, nc, ck = _plan(lib, sizes, k, h)
    assert rc == 0 and (nc, ck) == (2, 65)
    b = len(sizes)
    desc = table[:VL_DESC * b].reshape(b, VL_DESC)
    off = _offsets(sizes)
    for i, n in enumerate(sizes):
        assert desc[i][1] == off[i] and desc[i][2] == n
        assert desc[i][3] == i * k                                            # first Kp / output row: the FULL key count
        assert desc[i][4] == -(-n // ROWS)                                    # 32-row tiles
    slots = int(sum(int(d[9]) * int(d[7]) for d in desc))
    total = sum(sizes)
    assert ws == _r256(slots * _nkb(ck) * NCB * 4096) + _r256(nc * h * total * 8) + _r256(k * b * h * DK * 2)
    # the one-chunk plan equals the chunked plan at one chunk: the geometry depends on n and h only
    rc1, t1, ws1, nc1, ck1 = _plan(lib, sizes, ck, h)
    assert rc1 == 0 and (nc1, ck1) == (1, ck)
    d1 = t1[:VL_DESC * b].reshape(b, VL_DESC)
    assert np.array_equal(np.delete(d1, 3, axis=1), np.delete(desc, 3, axis=1)) and np.array_equal(t1[VL_DESC * b:], table[VL_DESC * b:])
    assert [int(d[3]) for d in d1] == [0, ck]
    assert ws1 == _r256(slots * _nkb(ck) * NCB * 4096) + _r256(ck * b * h * DK * 2)   # one chunk: no statistics area
    # the SimCLR recipe: 8 chunks of ceil(900 / 8) = 113 keys, the last one 900 - 7 x 113 = 109
    assert _plan(lib, sizes, 900, h, table=False)[3:] == (8, 113)
    # a bag of at most 1024 rows (32 tiles) is one workgroup per head (stored directly), a longer one is reduced
    rc, table, _, _, _ = _plan(lib, [1024, 1025], 100, 2)
    desc = table[:VL_DESC * 2].reshape(2, VL_DESC)
    assert rc == 0 and [int(d[10]) for d in desc] == [1, 0] and int(desc[0][9]) == 2


def test_predicates_and_switches(monkeypatch):
    from snuffy_amd import functional as SF
    from snuffy_amd import ops, packed
    ks = (0, 1, 128, 129, 900, 1024, 1025)
    want = [False, True, True, True, True, True, False]
    assert [ops.mfma_attn_dk256_supported(k) for k in ks] == want
    assert [ops.varlen_attn_dk256_supported(k) for k in ks] == want
    # the 32-bit element offsets of the family: rows, row pitch, rows x pitch
    assert ops.mfma_attn_dk256_supported(900, 0xffff00, 128) and not ops.mfma_attn_dk256_supported(900, 0xffff01, 128)
    assert ops.mfma_attn_dk256_supported(900, 100, (1 << 24) - 8) and not ops.mfma_attn_dk256_supported(900, 100, 1 << 24)
    assert ops.mfma_attn_dk256_supported(900, 2097151, 1024) and not ops.mfma_attn_dk256_supported(900, 2097152, 1024)
    # the older predicates keep their answers at this width
    for k in (1, 128, 200, 900):
        assert not ops.mfma_attn_supported(k, 256)
        assert not ops.varlen_attn_supported("bf16", k, 256)
        assert not ops.varlen_attn_chunks_supported("bf16", k, 256)
    assert SF.head_pad(256) is None and SF.packed_head_pad(256) is None
    for on in (True, False):
        monkeypatch.setattr(packed, "PACK_DK256", on)
        assert packed.dk256_ok("bf16", 512, 2, 900) is on                          # the SimCLR ResNet-18 recipe
        assert packed.dk256_ok("bf16", 256, 1, 1) is on and packed.dk256_ok("bf16", 768, 3, 1024) is on
        assert packed.dk256_ok("bf16", 512, 2, 1025) is False and packed.dk256_ok("bf16", 512, 2, 0) is False
        assert packed.dk256_ok("bf16", 512, 4, 900) is False                       # dk = 128: not this predicate's
        assert packed.dk256_ok("fp32", 512, 2, 900) is False                       # fp32 at this width: x3_dk256_ok
        assert packed.dk192_ok("bf16", 512, 2, 900) is False
        # fp32 is routed by its own switch, whatever this one says; neither consults the single-bag switch
        for x3_on in (True, False):
            monkeypatch.setattr(packed, "PACK_X3_DK256", x3_on)
            assert packed.x3_dk256_ok("fp32", 512, 2, 900) is x3_on and packed.x3_dk256_ok("bf16", 512, 2, 900) is False
        monkeypatch.setattr(SF, "MFMA_ATTN_DK256", not on)
        assert packed.dk256_ok("bf16", 512, 2, 900) is on


# (VGPRs, scratch bytes per lane) of the new kernels, sparse_attn_mfma_dk256_kernel<NKB, AUX, MODE, VL> (tools/scan_spills.py on the build
# that added them; DESIGN section 4 has the table).  No form spills, the varlen forms included: at bf16 the Kp fragments of a key block are
# 64 registers, half the fp32-class figure.
A256_TABLE = {
    # (nkb, aux, mode, varlen).  One launch (MODE 0), single bag and varlen:
    (1, False, 0, False): (228, 0), (1, True, 0, False): (232, 0), (2, False, 0, False): (288, 0), (2, True, 0, False): (292, 0),
    (4, False, 0, False): (420, 0), (4, True, 0, False): (420, 0),
    (1, False, 0, True): (240, 0), (1, True, 0, True): (244, 0), (2, False, 0, True): (308, 0), (2, True, 0, True): (308, 0),
    (4, False, 0, True): (436, 0), (4, True, 0, True): (436, 0),
    # statistics pass of a key chunk (MODE 1)
    (2, False, 1, False): (144, 0), (4, False, 1, False): (144, 0), (2, False, 1, True): (144, 0), (4, False, 1, True): (144, 0),
    # main pass of a key chunk (MODE 2)
    (2, False, 2, False): (288, 0), (2, True, 2, False): (292, 0), (4, False, 2, False): (416, 0), (4, True, 2, False): (420, 0),
    (2, False, 2, True): (308, 0), (2, True, 2, True): (308, 0), (4, False, 2, True): (436, 0), (4, True, 2, True): (436, 0),
}


def test_new_kernels_keep_their_registers_and_scratch():
    import scan_spills
    objdir = os.path.join(scan_spills.ROOT, "snuffy_amd", "build")
    if not os.path.isdir(objdir) or not os.path.exists(os.path.join(objdir, "sparse_attn_mfma_dk256.o")):
        pytest.skip("no build objects here (the library was built elsewhere)")
    try:
        ks = scan_spills.kernels(objdir)
    except RuntimeError as exc:
        pytest.skip(str(exc))
    names = scan_spills.demangle([k[1] for k in ks])
    got, reduce256 = {}, set()
    for (obj, _, scratch, spilled, vgpr), name in zip(ks, names):
        args = [a.strip() for a in name.split("<", 1)[1].split(">")[0].split(",")] if "<" in name else []
        if "sparse_attn_mfma_dk256_kernel<" in name:
            assert obj == ("sparse_attn_mfma_dk256.o" if args[2] == "0" else "sparse_attn_mfma_dk256_chunks.o"), (obj, name)
            assert spilled == 0, name
            got[(int(args[0]), args[1] == "true", int(args[2]), args[3] == "true")] = (vgpr, scratch)
        elif obj.startswith("sparse_attn_mfma_dk256") and "reduce_partials_kernel<256," in name:
            assert scratch == 0, name
            reduce256.add(int(args[1]))
        assert "sparse_attn_mfma_kernel<256," not in name and "sparse_attn_stats_kernel<256," not in name   # the older template stays without it
    assert all(s == 0 for (_, _, _, vl), (_, s) in got.items() if not vl)      # the condition: single-bag forms have zero scratch
    assert got == A256_TABLE
    assert reduce256 == {1, 2, 4}
