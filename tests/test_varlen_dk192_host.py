"""Packed (varlen) bf16 attention at head width 192 (the reference README's MAE recipe: D = 768, h = 4, Lambda = 500), the part that
needs no GPU: the plan entry point of the width (pure host code; cu_count() falls back to the MI355X's 256 without a device), the
predicates behind ``packed.pack_groups``, and the scratch bytes of the new kernels."""
import ctypes
import os
import sys

import numpy as np
import pytest

from snuffy_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

VL_DESC = 12
KMAX = 128
NCB = 6                                                                         # 32-wide column blocks of a dk = 192 output tile row


def _offsets(sizes):
    off = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum(sizes, out=off[1:])
    return off


def _plan(lib, sizes, k, h, table=True):
    """(rc, table, workspace bytes, chunks, keys per chunk)"""
    fn, off = lib.snf_sparse_attn_varlen_dk192_plan, _offsets(sizes)
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
    """The chunk rule of the single-bag driver at dk = 192 (make_chunks), for every k: the plan reports it, and every chunk (the
    shorter last one included) needs a key-block count the chunked varlen kernels are instantiated for."""
    lib = _ffi.load()
    seen = set()
    for k in range(1, 8 * KMAX + 1):
        rc, _, _, nc, ck = _plan(lib, [300, 5000], k, 2, table=False)
        assert rc == 0, k
        count = -(-k // KMAX)
        size = -(-k // count)
        assert (nc, ck) == (count, size), k
        for c in range(count):
            kc = min(size, k - c * size)
            assert 1 <= kc <= KMAX, (k, c)
            if count > 1:
                seen.add(_nkb(kc))
    assert seen == {2, 4}, seen


def test_refusals():
    lib = _ffi.load()
    assert _plan(lib, [1000, 2000], 8 * KMAX + 1, 4)[0] == _ffi.SNF_EUNSUPPORTED
    assert b"unsupported" in lib.snf_last_error()
    assert _plan(lib, [1000, 2000], 8 * KMAX, 4)[0] == 0
    off = np.array([0, 100, 100], dtype=np.int64)                             # an empty bag
    need = ctypes.c_size_t(0)
    assert lib.snf_sparse_attn_varlen_dk192_plan(ctypes.c_void_p(off.ctypes.data), 2, 300, 4, None, 0, ctypes.byref(need), None, None,
                                                 None) == _ffi.SNF_EUNSUPPORTED
    assert b"unsupported" in lib.snf_last_error()
    # the older plan functions keep refusing the width
    ws = ctypes.c_size_t(0)
    o2 = _offsets([1000, 2000])
    assert lib.snf_sparse_attn_varlen_plan(ctypes.c_void_p(o2.ctypes.data), 2, 100, 4, 192, None, 0, ctypes.byref(need),
                                           ctypes.byref(ws)) == _ffi.SNF_EUNSUPPORTED
    assert lib.snf_sparse_attn_varlen_chunked_plan(ctypes.c_void_p(o2.ctypes.data), 2, 500, 4, 192, None, 0, ctypes.byref(need),
                                                   ctypes.byref(ws), None, None) == _ffi.SNF_EUNSUPPORTED


def test_plan_of_the_smallest_chunked_case():
    lib = _ffi.load()
    sizes, k, h = [1000, 2000], 129, 4                                         # 65 + 64 keys: 4 and 2 key blocks
    rc, table, ws, nc, ck = _plan(lib, sizes, k, h)
    assert rc == 0 and (nc, ck) == (2, 65)
    b = len(sizes)
    desc = table[:VL_DESC * b].reshape(b, VL_DESC)
    off = _offsets(sizes)
    for i, n in enumerate(sizes):
        assert desc[i][1] == off[i] and desc[i][2] == n
        assert desc[i][3] == i * k                                            # first Kp / output row: the FULL key count
    slots = int(sum(int(d[9]) * int(d[7]) for d in desc))
    total = sum(sizes)
    assert ws >= slots * _nkb(ck) * NCB * 4096 + nc * h * total * 8
    # the geometry is the one-chunk plan's at the chunk size: it depends on n and h only
    rc1, t1, ws1, nc1, ck1 = _plan(lib, sizes, ck, h)
    assert rc1 == 0 and (nc1, ck1) == (1, ck)
    d1 = t1[:VL_DESC * b].reshape(b, VL_DESC)
    assert np.array_equal(np.delete(d1, 3, axis=1), np.delete(desc, 3, axis=1)) and np.array_equal(t1[VL_DESC * b:], table[VL_DESC * b:])
    assert [int(d[3]) for d in d1] == [0, ck]
    # one chunk: no statistics area -- partial tiles (+ the staging of an f32 Kp, 2 bytes per element rounded up to 256)
    staging = (ck * b * h * 192 * 2 + 255) // 256 * 256
    assert ws1 == slots * _nkb(ck) * NCB * 4096 + staging
    # a bag of at most 1024 rows is one workgroup per head (stored directly), a longer one is reduced
    rc, table, _, _, _ = _plan(lib, [1024, 1025], 100, 4)
    desc = table[:VL_DESC * 2].reshape(2, VL_DESC)
    assert rc == 0 and [int(d[10]) for d in desc] == [1, 0] and int(desc[0][9]) == 4


def test_predicates_behind_pack_groups(monkeypatch):
    from snuffy_amd import functional as SF
    from snuffy_amd import ops, packed
    assert [ops.varlen_attn_dk192_supported(k) for k in (0, 1, 128, 129, 1024, 1025)] == [False, True, True, True, True, False]
    # the older predicates keep their answers at this width
    for kind in ("bf16", "fp32"):
        for k in (1, 128, 200, 500):
            assert not ops.varlen_attn_supported(kind, k, 192)
            assert not ops.varlen_attn_chunks_supported(kind, k, 192)
    assert SF.packed_head_pad(192) is None
    assert isinstance(packed.PACK_DK192, bool)
    for on in (True, False):
        monkeypatch.setattr(packed, "PACK_DK192", on)
        assert packed.dk192_ok("bf16", 768, 4, 500) is on                         # the MAE recipe
        assert packed.dk192_ok("bf16", 384, 2, 1) is on and packed.dk192_ok("bf16", 768, 4, 1024) is on
        assert packed.dk192_ok("bf16", 768, 4, 1025) is False and packed.dk192_ok("bf16", 768, 4, 0) is False
        assert packed.dk192_ok("bf16", 768, 6, 500) is False                      # dk = 128: not this predicate's
        assert packed.dk192_ok("fp32", 768, 4, 500) is False                      # stays per bag whatever the switch
        for kind in ("bf16", "fp32"):                                             # PACK_KEY_CHUNKS does not take the width either way
            assert not packed.key_chunks_ok([], kind, 768, 4, 500, 5, 9000)


# Scratch bytes per lane of the new kernels (tools/scan_spills.py on the build that added them; DESIGN section 4 lists them):
# sparse_attn_mfma_vl192_kernel<192, NKB, unsigned short, AUX, EXT, 8, VL = true> -- (nkb, aux, ext) -- and
# sparse_attn_stats_vl192_kernel<192, NKB, unsigned short, VL = true>.  Nothing spills but the key-chunked forward at 4 key blocks with
# A | lse: one register, saved in the prologue and read back on the once-per-head Kp commit of the pooling waves.
MFMA_SCRATCH = {(1, False, False): 0, (1, True, False): 0, (2, False, False): 0, (2, True, False): 0, (4, False, False): 0,
                (4, True, False): 0, (2, False, True): 0, (2, True, True): 0, (4, False, True): 0, (4, True, True): 8}
STATS_SCRATCH = {2: 0, 4: 0}


def test_new_kernels_keep_their_scratch():
    import scan_spills
    objdir = os.path.join(scan_spills.ROOT, "snuffy_amd", "build")
    if not os.path.isdir(objdir) or not os.path.exists(os.path.join(objdir, "sparse_attn_mfma_varlen_dk192.o")):
        pytest.skip("no build objects here (the library was built elsewhere)")
    try:
        ks = scan_spills.kernels(objdir)
    except RuntimeError as exc:
        pytest.skip(str(exc))
    names = scan_spills.demangle([k[1] for k in ks])
    mfma, stats, old = {}, {}, {"fwd": 0, "stats": 0, "bwd": 0}
    for (obj, _, scratch, _, _), name in zip(ks, names):
        args = [a.strip() for a in name.split("<", 1)[1].split(">")[0].split(",")] if "<" in name else []
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
