"""Fused fp32-class (split-bf16 x 3) attention at head width 256 (the reference README's SimCLR ResNet-18 recipe: D = 512, h = 2,
Lambda = 900 as 200 + 700), the part that needs no GPU: the plan entry points of the width (pure host code; cu_count() falls back to the
MI355X's 256 without a device), the predicates and switches behind ``functional.encoder_layer`` / ``packed.pack_groups``, and the scratch
bytes of the new kernels."""
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


def _offsets(sizes):
    off = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum(sizes, out=off[1:])
    return off


def _plan(lib, sizes, k, h, table=True):
    """(rc, table, workspace bytes, chunks, keys per chunk)"""
    fn, off = lib.snf_sparse_attn_x3_varlen_dk256_plan, _offsets(sizes)
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


def test_every_key_count_has_built_chunks():
    """The chunk rule (ceil(k / chunks) keys rounded up to a multiple of 4, the last chunk shorter), for every k: the plan reports it,
    the chunks cover k, and every chunk of a chunked launch needs a key-block count the MODE 1 / MODE 2 kernels are instantiated for."""
    lib = _ffi.load()
    seen = set()
    for k in range(1, MAX_CHUNKS * KMAX + 1):
        rc, _, _, nc, ck = _plan(lib, [300, 5000], k, 2, table=False)
        assert rc == 0, k
        assert nc == -(-k // KMAX), k
        assert 1 <= ck <= KMAX and (nc - 1) * ck < k <= nc * ck, (k, nc, ck)
        assert lib.snf_sparse_attn_fwd_x3_dk256_workspace_bytes(300, k, 2) > 0, k      # the single-bag plan takes the same chunks
        if nc == 1:
            assert ck == k
            continue
        assert ck % 4 == 0, (k, ck)
        for c in range(nc):
            kc = min(ck, k - c * ck)
            assert 1 <= kc <= KMAX, (k, c)
            seen.add(_nkb(kc))
    assert seen == {2, 4}, seen                                                # the counts sparse_attn_x3_dk256_chunks.hip builds


def test_refusals():
    lib = _ffi.load()
    assert _plan(lib, [1000, 2000], MAX_CHUNKS * KMAX + 1, 2)[0] == _ffi.SNF_EUNSUPPORTED
    assert b"unsupported" in lib.snf_last_error()
    assert _plan(lib, [1000, 2000], 0, 2)[0] == _ffi.SNF_EUNSUPPORTED
    assert b"unsupported" in lib.snf_last_error()
    assert _plan(lib, [1000, 2000], MAX_CHUNKS * KMAX, 2)[0] == 0
    off = np.array([0, 100, 100], dtype=np.int64)                             # an empty bag
    need = ctypes.c_size_t(0)
    assert lib.snf_sparse_attn_x3_varlen_dk256_plan(ctypes.c_void_p(off.ctypes.data), 2, 300, 2, None, 0, ctypes.byref(need), None, None,
                                                    None) == _ffi.SNF_EUNSUPPORTED
    assert b"unsupported" in lib.snf_last_error()
    # the plan and workspace functions of dk = 64 / 128 keep refusing the width
    ws = ctypes.c_size_t(0)
    o2 = _offsets([1000, 2000])
    assert lib.snf_sparse_attn_x3_varlen_plan(ctypes.c_void_p(o2.ctypes.data), 2, 100, 2, 256, None, 0, ctypes.byref(need),
                                              ctypes.byref(ws)) == _ffi.SNF_EUNSUPPORTED
    assert lib.snf_sparse_attn_x3_varlen_chunked_plan(ctypes.c_void_p(o2.ctypes.data), 2, 900, 2, 256, None, 0, ctypes.byref(need),
                                                      ctypes.byref(ws), None, None) == _ffi.SNF_EUNSUPPORTED
    assert lib.snf_sparse_attn_fwd_x3_workspace_bytes(4096, 100, 2, 256) == 0
    assert lib.snf_sparse_attn_fwd_x3_workspace_bytes(4096, 900, 2, 256) == 0
    # the entry points of 192 take no width: a dk = 256 operand does not fit their row pitch of h * 192, and their answers for (n, k, h)
    # are the pinned ones (tests/golden/attn_plans.npz) -- what they must not do is follow the new family's geometry
    n, k, h = 3000, 900, 2
    w192 = lib.snf_sparse_attn_fwd_x3_dk192_workspace_bytes(n, k, h)
    assert w192 == -(-n // 64) * h * 2 * 4 * 6 * 4096 + 8 * h * n * 8         # 64-row tiles, 6 column blocks: its own closed form
    assert w192 != lib.snf_sparse_attn_fwd_x3_dk256_workspace_bytes(n, k, h)


def test_single_bag_workspace_follows_the_predicate():
    from snuffy_amd import ops
    lib = _ffi.load()
    for k in (-1, 0, 1, 20, 128, 129, 900, 1024, 1025, 4096):
        assert (lib.snf_sparse_attn_fwd_x3_dk256_workspace_bytes(3000, k, 2) > 0) == ops.x3_attn_dk256_supported(k), k
    assert lib.snf_sparse_attn_fwd_x3_dk256_workspace_bytes(0, 100, 2) == 0
    assert lib.snf_sparse_attn_fwd_x3_dk256_workspace_bytes(3000, 100, 0) == 0
    # chunked: partial tiles at the largest chunk's 4 key blocks, one (max, sum) pair per chunk, head and row
    n, k, h = 3000, 900, 2
    tiles = -(-n // ROWS) * h                                                  # 188 < 256 CUs: one tile per workgroup, two segments
    chunks = -(-k // KMAX)                                                     # 8 chunks of 116 keys (the last 88): 4 key blocks
    assert lib.snf_sparse_attn_fwd_x3_dk256_workspace_bytes(n, k, h) == tiles * 2 * 4 * NCB * 4096 + chunks * h * n * 8


def test_plan_geometry():
    lib = _ffi.load()
    sizes, k, h = [1000, 2000], 129, 2                                         # 68 + 61 keys: 4 and 2 key blocks
    rc, table, ws, nc, ck = _plan(lib, sizes, k, h)
    assert rc == 0 and (nc, ck) == (2, 68)
    b = len(sizes)
    desc = table[:VL_DESC * b].reshape(b, VL_DESC)
    off = _offsets(sizes)
    for i, n in enumerate(sizes):
        assert desc[i][1] == off[i] and desc[i][2] == n
        assert desc[i][3] == i * k                                            # first Kp / output row: the FULL key count
        assert desc[i][4] == -(-n // ROWS)                                    # 32-row tiles
    slots = int(sum(int(d[9]) * int(d[7]) for d in desc))
    total = sum(sizes)
    assert ws == slots * _nkb(ck) * NCB * 4096 + nc * h * total * 8
    # the geometry is the one-chunk plan's at the chunk size: it depends on n and h only
    rc1, t1, ws1, nc1, ck1 = _plan(lib, sizes, ck, h)
    assert rc1 == 0 and (nc1, ck1) == (1, ck)
    d1 = t1[:VL_DESC * b].reshape(b, VL_DESC)
    assert np.array_equal(np.delete(d1, 3, axis=1), np.delete(desc, 3, axis=1)) and np.array_equal(t1[VL_DESC * b:], table[VL_DESC * b:])
    assert [int(d[3]) for d in d1] == [0, ck]
    assert ws1 == slots * _nkb(ck) * NCB * 4096                               # one chunk: no statistics area
    # the SimCLR recipe: 8 chunks of ceil(900 / 8) = 113 -> 116 keys, the last one 900 - 7 x 116 = 88
    assert _plan(lib, sizes, 900, h, table=False)[3:] == (8, 116)
    # a bag of at most 1024 rows (32 tiles) is one workgroup per head (stored directly), a longer one is reduced
    rc, table, _, _, _ = _plan(lib, [1024, 1025], 100, 2)
    desc = table[:VL_DESC * 2].reshape(2, VL_DESC)
    assert rc == 0 and [int(d[10]) for d in desc] == [1, 0] and int(desc[0][9]) == 2


def test_predicates_and_switches(monkeypatch):
    from snuffy_amd import functional as SF
    from snuffy_amd import ops, packed
    assert [ops.x3_attn_dk256_supported(k) for k in (0, 1, 128, 129, 900, 1024, 1025)] == [False, True, True, True, True, True, False]
    assert [ops.varlen_attn_x3_dk256_supported(k) for k in (0, 1, 128, 129, 900, 1024, 1025)] == [False, True, True, True, True, True,
                                                                                                False]
    # the older predicates keep their answers at this width
    for k in (1, 128, 200, 900):
        assert not ops.x3_attn_supported(k, 256)
        assert not ops.varlen_attn_supported("fp32", k, 256)
        assert not ops.varlen_attn_chunks_supported("fp32", k, 256)
        assert ops.x3u_attn_supported(k, 256)
    assert SF.head_pad(256) is None and SF.packed_head_pad(256) is None
    # the verdicts of profiles/x3_dk256.txt: the single bag stays on the unfused pair, packed bags take the new kernel
    assert SF.X3_ATTN_DK256 is False and packed.PACK_X3_DK256 is True
    for on in (True, False):
        monkeypatch.setattr(packed, "PACK_X3_DK256", on)
        assert packed.x3_dk256_ok("fp32", 512, 2, 900) is on                      # the SimCLR ResNet-18 recipe
        assert packed.x3_dk256_ok("fp32", 256, 1, 1) is on and packed.x3_dk256_ok("fp32", 768, 3, 1024) is on
        assert packed.x3_dk256_ok("fp32", 512, 2, 1025) is False and packed.x3_dk256_ok("fp32", 512, 2, 0) is False
        assert packed.x3_dk256_ok("fp32", 512, 4, 900) is False                   # dk = 128: not this predicate's
        assert packed.x3_dk256_ok("bf16", 512, 2, 900) is False                   # bf16 at this width is not built
        assert packed.x3_dk192_ok("fp32", 512, 2, 900) is False and packed.dk192_ok("bf16", 512, 2, 900) is False
        # the single-bag switch is not consulted
        monkeypatch.setattr(SF, "X3_ATTN_DK256", not on)
        assert packed.x3_dk256_ok("fp32", 512, 2, 900) is on


# Scratch bytes per lane of the new kernels, sparse_attn_x3_dk256_kernel<NKB, AUX, MODE, VL> (tools/scan_spills.py on the build that added
# them; DESIGN section 4 lists them with the register counts).  Only the varlen forms at 4 key blocks spill: they hold 128 accumulators
# and the 128 Kp registers next to the bag's descriptor words.
X3Y_SCRATCH = {
    # (nkb, aux, mode, varlen): bytes.  One launch (MODE 0), single bag and varlen:
    (1, False, 0, False): 0, (1, True, 0, False): 0, (2, False, 0, False): 0, (2, True, 0, False): 0,
    (4, False, 0, False): 0, (4, True, 0, False): 0,
    (1, False, 0, True): 0, (1, True, 0, True): 0, (2, False, 0, True): 0, (2, True, 0, True): 0,
    (4, False, 0, True): 72, (4, True, 0, True): 84,
    # statistics pass of a key chunk (MODE 1)
    (2, False, 1, False): 0, (4, False, 1, False): 0, (2, False, 1, True): 0, (4, False, 1, True): 0,
    # main pass of a key chunk (MODE 2)
    (2, False, 2, False): 0, (2, True, 2, False): 0, (4, False, 2, False): 0, (4, True, 2, False): 0,
    (2, False, 2, True): 0, (2, True, 2, True): 0, (4, False, 2, True): 72, (4, True, 2, True): 84,
}


def test_new_kernels_keep_their_scratch():
    import scan_spills
    objdir = os.path.join(scan_spills.ROOT, "snuffy_amd", "build")
    if not os.path.isdir(objdir) or not os.path.exists(os.path.join(objdir, "sparse_attn_x3_dk256.o")):
        pytest.skip("no build objects here (the library was built elsewhere)")
    try:
        ks = scan_spills.kernels(objdir)
    except RuntimeError as exc:
        pytest.skip(str(exc))
    names = scan_spills.demangle([k[1] for k in ks])
    got, reduce256 = {}, set()
    for (obj, _, scratch, _, _), name in zip(ks, names):
        args = [a.strip() for a in name.split("<", 1)[1].split(">")[0].split(",")] if "<" in name else []
        if "sparse_attn_x3_dk256_kernel<" in name:
            assert obj == ("sparse_attn_x3_dk256.o" if args[2] == "0" else "sparse_attn_x3_dk256_chunks.o"), (obj, name)
            got[(int(args[0]), args[1] == "true", int(args[2]), args[3] == "true")] = scratch
        elif "x3_reduce_kernel<256," in name:
            assert scratch == 0, name
            reduce256.add(int(args[1]))
        assert "sparse_attn_x3_kernel<256," not in name                          # the 64 / 128 family stays without the width
    assert got == X3Y_SCRATCH
    assert reduce256 == {1, 2, 4}
