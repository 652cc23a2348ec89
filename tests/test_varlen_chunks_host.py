"""Packed (varlen) attention above one key chunk and at padded head widths, the part that needs no GPU: the chunked plan entry points
(pure host code; cu_count() falls back to the MI355X's 256 without a device), the predicates behind ``packed.pack_groups``, and the
scratch bytes of the new kernel instantiations."""
import ctypes
import os
import sys

import numpy as np
import pytest

from snuffy_amd import _ffi
from tests.attn_widths import _offsets
from tests.attn_widths import nkb_of_family as _nkb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

VL_DESC = 12
OLD = {"mfma": "snf_sparse_attn_varlen_plan", "x3": "snf_sparse_attn_x3_varlen_plan"}
NEW = {"mfma": "snf_sparse_attn_varlen_chunked_plan", "x3": "snf_sparse_attn_x3_varlen_chunked_plan"}
KMAX = {128: 224, 64: 256}


def _old_plan(lib, fam, sizes, k, h, dk):
    fn, off = getattr(lib, OLD[fam]), _offsets(sizes)
    need, ws = ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = fn(ctypes.c_void_p(off.ctypes.data), len(sizes), k, h, dk, None, 0, ctypes.byref(need), ctypes.byref(ws))
    if rc:
        return rc, None, None
    table = np.full(need.value, -7, dtype=np.int32)
    assert fn(ctypes.c_void_p(off.ctypes.data), len(sizes), k, h, dk, ctypes.c_void_p(table.ctypes.data), table.size,
              ctypes.byref(need), ctypes.byref(ws)) == 0
    return 0, table, ws.value


def _new_plan(lib, fam, sizes, k, h, dk, table=True):
    """(rc, table, workspace bytes, chunks, keys per chunk)"""
    fn, off = getattr(lib, NEW[fam]), _offsets(sizes)
    need, ws, nc, ck = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = fn(ctypes.c_void_p(off.ctypes.data), len(sizes), k, h, dk, None, 0, ctypes.byref(need), ctypes.byref(ws), ctypes.byref(nc),
            ctypes.byref(ck))
    if rc or not table:
        return rc, None, ws.value, nc.value, ck.value
    tab = np.full(need.value, -7, dtype=np.int32)
    assert fn(ctypes.c_void_p(off.ctypes.data), len(sizes), k, h, dk, ctypes.c_void_p(tab.ctypes.data), tab.size, ctypes.byref(need),
              ctypes.byref(ws), None, None) == 0                              # the chunk outputs are nullable
    return 0, tab, ws.value, nc.value, ck.value


@pytest.mark.parametrize("fam,keys", [("mfma", 113), ("x3", 116)])
def test_chunked_plan_of_the_smallest_chunked_case(fam, keys):
    lib = _ffi.load()
    sizes, k, h, dk = [1000, 2000], 225, 6, 128
    rc, table, ws, nc, ck = _new_plan(lib, fam, sizes, k, h, dk)
    assert rc == 0 and (nc, ck) == (2, keys)
    b = len(sizes)
    desc = table[:VL_DESC * b].reshape(b, VL_DESC)
    off = _offsets(sizes)
    for i, n in enumerate(sizes):
        assert desc[i][3] == i * k                                            # first Kp / output row: the FULL key count
        assert desc[i][1] == off[i] and desc[i][2] == n
    slots = int(sum(int(d[9]) * int(d[7]) for d in desc))
    total = sum(sizes)
    assert ws >= slots * _nkb(fam, ck, dk) * (dk // 32) * 4096 + nc * h * total * 8
    # the geometry is the one-chunk plan's at the chunk size: it depends on n and h only
    rc1, t1, _ = _old_plan(lib, fam, sizes, ck, h, dk)
    assert rc1 == 0
    d1 = t1[:VL_DESC * b].reshape(b, VL_DESC)
    assert np.array_equal(np.delete(d1, 3, axis=1), np.delete(desc, 3, axis=1)) and np.array_equal(t1[VL_DESC * b:], table[VL_DESC * b:])


@pytest.mark.parametrize("fam", ["mfma", "x3"])
def test_chunk_counts_workspace_and_refusals(fam):
    lib = _ffi.load()
    sizes, h = [1000, 2000], 6
    assert _new_plan(lib, fam, sizes, 257, h, 64)[3] == 2
    rc, table, ws, nc, ck = _new_plan(lib, fam, sizes, 900, 4, 128)
    assert rc == 0 and (nc, ck) == (5, 180)
    desc = table[:VL_DESC * 2].reshape(2, VL_DESC)
    assert [int(d[3]) for d in desc] == [0, 900]
    slots = int(sum(int(d[9]) * int(d[7]) for d in desc))
    assert ws >= slots * _nkb(fam, 180, 128) * 4 * 4096 + 5 * 4 * 3000 * 8
    # one chunk: the table of the existing plan, integer for integer
    rc, table, ws, nc, ck = _new_plan(lib, fam, sizes, 200, h, 128)
    rc0, t0, ws0 = _old_plan(lib, fam, sizes, 200, h, 128)
    assert rc == 0 and rc0 == 0 and (nc, ck) == (1, 200) and np.array_equal(table, t0) and ws >= ws0
    # refusals
    assert _new_plan(lib, fam, sizes, 8 * 224 + 1, h, 128)[0] == _ffi.SNF_EUNSUPPORTED
    assert _new_plan(lib, fam, sizes, 8 * 224, h, 128)[0] == 0
    assert _new_plan(lib, fam, sizes, 8 * 256 + 1, h, 64)[0] == _ffi.SNF_EUNSUPPORTED
    assert _new_plan(lib, fam, sizes, 200, h, 192)[0] == _ffi.SNF_EUNSUPPORTED
    assert _new_plan(lib, fam, sizes, 500, h, 192)[0] == _ffi.SNF_EUNSUPPORTED
    assert _new_plan(lib, fam, sizes, 200, h, 83)[0] == _ffi.SNF_EUNSUPPORTED
    off = np.array([0, 100, 100], dtype=np.int64)                             # an empty bag
    need = ctypes.c_size_t(0)
    assert getattr(lib, NEW[fam])(ctypes.c_void_p(off.ctypes.data), 2, 300, h, 128, None, 0, ctypes.byref(need), None, None,
                                  None) == _ffi.SNF_EUNSUPPORTED
    assert b"unsupported" in lib.snf_last_error()
    # the existing plan functions keep refusing more than one chunk
    assert _old_plan(lib, fam, sizes, 225, h, 128)[0] != 0 and _old_plan(lib, fam, sizes, 257, h, 64)[0] != 0


@pytest.mark.parametrize("fam", ["mfma", "x3"])
@pytest.mark.parametrize("dk", [64, 128])
def test_every_key_count_has_built_chunks(fam, dk):
    """The chunk rule of the family's single-bag driver, for every k: the plan reports it, and every chunk (the shorter last one
    included) needs a key-block count the chunked varlen kernels are instantiated for."""
    lib = _ffi.load()
    kmax = KMAX[dk]
    built = {4, 6, 7, 8} if fam == "mfma" else {4, 7, 8}
    if dk == 128:
        built.discard(8)
    seen = set()
    for k in range(1, 8 * kmax + 1):
        rc, _, _, nc, ck = _new_plan(lib, fam, [300, 5000], k, 2, dk, table=False)
        assert rc == 0, k
        count = -(-k // kmax)
        size = -(-k // count)
        if fam == "x3" and count > 1:
            size = (size + 3) & ~3
        assert (nc, ck) == (count, size), k
        if count > 1:
            for c in range(count):
                kc = min(size, k - c * size)
                assert kc >= 1, (k, c)
                seen.add(_nkb(fam, kc, dk))
    assert seen == built, (seen, built)


def test_predicates_behind_pack_groups(monkeypatch):
    from snuffy_amd import functional as SF
    from snuffy_amd import ops, packed
    for kind in ("bf16", "fp32"):
        for dk, kmax in KMAX.items():
            for k in (1, kmax, kmax + 1, 8 * kmax):
                assert ops.varlen_attn_chunks_supported(kind, k, dk), (k, dk)
                assert ops.varlen_attn_supported(kind, k, dk) == (k <= kmax)       # keeps its meaning of one chunk
            assert not ops.varlen_attn_chunks_supported(kind, 8 * kmax + 1, dk)
            assert not ops.varlen_attn_chunks_supported(kind, 0, dk)
        for dk in (32, 83, 96, 192):
            assert not ops.varlen_attn_chunks_supported(kind, 200, dk)
    # padding on the packed path: only between the kernels' widths
    assert [SF.packed_head_pad(dk) for dk in (64, 80, 96, 112, 128)] == [64, 128, 128, 128, 128]
    assert all(SF.packed_head_pad(dk) is None for dk in (16, 32, 48, 63, 83, 100, 144, 192))
    assert isinstance(packed.PACK_KEY_CHUNKS, bool)

    class _Lin:
        def __init__(self):
            import torch
            self.weight = torch.zeros(4, 4)

    class _Layer:
        def __init__(self, f):
            import torch
            self.self_attn = type("A", (), {"linears": [_Lin(), _Lin(), _Lin(), _Lin()]})()
            self.feed_forward = type("F", (), {"w_2": type("W", (), {"weight": torch.zeros(4, f)})()})()
    layers = [_Layer(1536)]
    for on in (True, False):
        monkeypatch.setattr(packed, "PACK_KEY_CHUNKS", on)
        for kind in ("bf16", "fp32"):
            assert packed.key_chunks_ok(layers, kind, 384, 4, 900, 5, 9000) is on       # the README recipes: dk = 96 -> 128
            assert packed.key_chunks_ok(layers, kind, 384, 4, 500, 64, 64000) is on
            assert packed.key_chunks_ok(layers, kind, 768, 6, 448, 5, 9000) is on       # dk = 128, two chunks
            assert not packed.key_chunks_ok(layers, kind, 768, 4, 500, 5, 9000)         # dk = 192 stays per bag
            assert not packed.key_chunks_ok(layers, kind, 192, 4, 300, 5, 9000)         # dk = 48: not padded on the packed path
            assert not packed.key_chunks_ok(layers, kind, 768, 6, 8 * 224 + 1, 5, 90000)
            assert not packed.key_chunks_ok(layers, kind, 392, 4, 300, 5, 9000)         # dk = 98: no padded form
    monkeypatch.setattr(packed, "PACK_KEY_CHUNKS", True)
    monkeypatch.setattr(SF, "FP32_GEMM", "library")                                     # the padded projections are split-bf16 GEMMs
    assert not packed.key_chunks_ok(layers, "fp32", 384, 4, 500, 5, 9000)
    assert packed.key_chunks_ok(layers, "fp32", 768, 6, 448, 5, 9000)


# Scratch bytes per lane of the new instantiations (tools/scan_spills.py on the build that added them; DESIGN section 4 has the table).
# fp32-class: sparse_attn_x3_kernel<DK, NKB, AUX, MODE, VL = true> -- (dk, nkb, aux, mode).  bf16: sparse_attn_mfma_kernel<DK, NKB,
# unsigned short, AUX, EXT = true, 8, VL = true> -- (dk, nkb, aux), and sparse_attn_stats_kernel<DK, NKB, unsigned short, VL = true>.
# What spills, spills as the single-chunk varlen instantiation of the same key-block count does (dk = 128 at 4 / 6 / 7 key blocks,
# dk = 64 at 7 / 8): values saved in the prologue and read back once per tile, no scratch stores inside the tile loop.
X3_SCRATCH = {(64, 4, False, 1): 0, (64, 4, False, 2): 0, (64, 4, True, 2): 0, (64, 7, False, 1): 0, (64, 7, False, 2): 0,
              (64, 7, True, 2): 0, (64, 8, False, 1): 0, (64, 8, False, 2): 0, (64, 8, True, 2): 0, (128, 4, False, 1): 0,
              (128, 4, False, 2): 100, (128, 4, True, 2): 116, (128, 7, False, 1): 0, (128, 7, False, 2): 500, (128, 7, True, 2): 508}
MFMA_SCRATCH = {(64, 4, False): 0, (64, 4, True): 0, (64, 6, False): 0, (64, 6, True): 0, (64, 7, False): 100, (64, 7, True): 100,
                (64, 8, False): 88, (64, 8, True): 84, (128, 4, False): 156, (128, 4, True): 156, (128, 6, False): 588,
                (128, 6, True): 588, (128, 7, False): 800, (128, 7, True): 828}
STATS_SCRATCH = {(64, 4): 0, (64, 6): 0, (64, 7): 0, (64, 8): 0, (128, 4): 0, (128, 6): 0, (128, 7): 0}


def test_new_instantiations_keep_their_scratch():
    import scan_spills
    objdir = os.path.join(scan_spills.ROOT, "snuffy_amd", "build")
    if not os.path.isdir(objdir) or not os.path.exists(os.path.join(objdir, "sparse_attn_x3_varlen_chunks.o")):
        pytest.skip("no build objects here (the library was built elsewhere)")
    try:
        ks = scan_spills.kernels(objdir)
    except RuntimeError as exc:
        pytest.skip(str(exc))
    names = scan_spills.demangle([k[1] for k in ks])
    x3, mfma, stats = {}, {}, {}
    for (obj, _, scratch, _, _), name in zip(ks, names):
        if "_varlen_chunks" not in obj:
            continue
        args = [a.strip() for a in name.split("<", 1)[1].split(">")[0].split(",")] if "<" in name else []
        if "sparse_attn_x3_kernel<" in name:
            assert args[4] == "true" and args[3] in ("1", "2"), name
            x3[(int(args[0]), int(args[1]), args[2] == "true", int(args[3]))] = scratch
        elif "sparse_attn_mfma_kernel<" in name:
            assert args[2] == "unsigned short" and args[4] == "true" and args[6] == "true", name
            mfma[(int(args[0]), int(args[1]), args[3] == "true")] = scratch
        elif "sparse_attn_stats_kernel<" in name:
            assert args[3] == "true", name
            stats[(int(args[0]), int(args[1]))] = scratch
    assert x3 == X3_SCRATCH
    assert mfma == MFMA_SCRATCH
    assert stats == STATS_SCRATCH
