"""Everything the host-only entry points of the tiled sparse-attention forward return, for a fixed list of cases: the eight varlen plan
functions (return code, both sizes, chunk count and size, the whole table, the snf_last_error() text of a refusal) and the five
single-bag workspace functions.  tests/test_attn_plan_golden.py replays the same cases against the built library and compares field
by field with tests/golden/attn_plans.npz.

    python tools/record_attn_plans.py path/to/libsnuffy_hip.so     # writes tests/golden/attn_plans.npz

Record the fixture with a library built from the commit BEFORE a change to the drivers, never from the code under test.  The plans
depend on the CU count; without a device the library assumes the MI355X's 256."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "attn_plans.npz")

# (entry point, takes dk, reports chunks, widths to ask for); new rows go at the END of both lists: the recorded cases keep their order
PLANS = [("snf_sparse_attn_varlen_plan", True, False, (64, 128, 192, 83)),
         ("snf_sparse_attn_varlen_chunked_plan", True, True, (64, 128, 192, 83)),
         ("snf_sparse_attn_varlen_dk192_plan", False, True, (192,)),
         ("snf_sparse_attn_x3_varlen_plan", True, False, (64, 128, 192, 83)),
         ("snf_sparse_attn_x3_varlen_chunked_plan", True, True, (64, 128, 192, 83)),
         ("snf_sparse_attn_x3_varlen_dk192_plan", False, True, (192,)),
         ("snf_sparse_attn_x3_varlen_dk256_plan", False, True, (256,)),
         ("snf_sparse_attn_varlen_dk256_plan", False, True, (256,))]
KMAX = {64: 256, 128: 224, 192: 128, 256: 128, 83: 224}
LONG = 256 * 16 * 128 + 1                                  # more than 256 * 16 tiles of either family (128 | 64 rows)
BATCH = [200, 1100, 2100]
BAGS = [[1], [1024], [1025], [1, 1024, 1025], [LONG], [300, LONG, 7], None]    # None: an empty bag, offsets [0, 100, 100]
# (entry point, takes dk, further arguments, the width of an entry point that takes none)
WORKSPACES = [("snf_sparse_attn_fwd_workspace_bytes", True, (1,), None), ("snf_sparse_attn_fwd_x3_workspace_bytes", True, (), None),
              ("snf_sparse_attn_fwd_x3_dk192_workspace_bytes", False, (), 192),
              ("snf_sparse_attn_fwd_x3_dk256_workspace_bytes", False, (), 256),
              ("snf_sparse_attn_fwd_mfma_dk256_workspace_bytes", False, (), 256)]


def _keys(dk):
    """0, one chunk, kmax and kmax + 1, two chunks whose last has another key-block count than the first (dk = 128: 257 = 132 + 125
    keys, 7 and 4 blocks; dk = 192: 129 = 68 + 61 keys, 4 and 2 blocks), three and eight chunks, 8 kmax and 8 kmax + 1."""
    kmax = KMAX[dk]
    return [0, 1, 100, kmax, kmax + 1, 129, 225, 257, 600, 7 * kmax + 1, 8 * kmax, 8 * kmax + 1]


def plan_cases():
    for name, has_dk, has_chunks, widths in PLANS:
        for dk in widths:
            for h in (1, 6):
                for k in _keys(dk):
                    yield name, has_dk, has_chunks, dk, h, k, BATCH
            for sizes in BAGS:
                for k in (100, KMAX[dk] + 1, 8 * KMAX[dk]):
                    yield name, has_dk, has_chunks, dk, 6, k, sizes


def _offsets(sizes):
    if sizes is None:
        return np.array([0, 100, 100], dtype=np.int64)
    off = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum(sizes, out=off[1:])
    return off


def _err(lib, rc):
    return lib.snf_last_error().decode() if rc else ""


def run(lib):
    """dict of arrays: one row per case."""
    lib.snf_last_error.restype = ctypes.c_char_p
    for name, _, _, _ in PLANS:
        getattr(lib, name).restype = ctypes.c_int
    for name, _, _, _ in WORKSPACES:
        getattr(lib, name).restype = ctypes.c_size_t
    case, rc_, need_, ws_, nc_, ck_, err_, short_rc, short_err, tab_len, tabs = [], [], [], [], [], [], [], [], [], [], []
    for name, has_dk, has_chunks, dk, h, k, sizes in plan_cases():
        fn, off = getattr(lib, name), _offsets(sizes)
        need, ws, nc, ck = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_int(-1), ctypes.c_int(-1)

        def call(table, ints):
            args = [ctypes.c_void_p(off.ctypes.data), ctypes.c_int(len(off) - 1), ctypes.c_int(k), ctypes.c_int(h)]
            args += [ctypes.c_int(dk)] if has_dk else []
            args += [ctypes.c_void_p(table.ctypes.data) if table is not None else None, ctypes.c_size_t(ints), ctypes.byref(need),
                     ctypes.byref(ws)]
            args += [ctypes.byref(nc), ctypes.byref(ck)] if has_chunks else []
            return fn(*args)
        rc = call(None, 0)
        case.append("%s dk=%d h=%d k=%d bags=%s" % (name, dk, h, k, "empty" if sizes is None else sizes))
        rc_.append(rc), err_.append(_err(lib, rc))
        need_.append(need.value), ws_.append(ws.value), nc_.append(nc.value), ck_.append(ck.value)
        table = np.full(need.value if rc == 0 else 0, -7, dtype=np.int32)
        if rc == 0:
            src = call(table, table.size - 1)                                  # a table buffer one int too short
            short_rc.append(src), short_err.append(_err(lib, src))
            assert call(table, table.size) == 0, case[-1]
        else:
            short_rc.append(0), short_err.append("")
        tab_len.append(table.size), tabs.append(table)
    out = {"plan_case": np.array(case), "plan_rc": np.array(rc_, dtype=np.int64), "plan_error": np.array(err_),
           "plan_table_ints": np.array(need_, dtype=np.uint64), "plan_workspace_bytes": np.array(ws_, dtype=np.uint64),
           "plan_n_chunks": np.array(nc_, dtype=np.int64), "plan_chunk_k": np.array(ck_, dtype=np.int64),
           "plan_short_table_rc": np.array(short_rc, dtype=np.int64), "plan_short_table_error": np.array(short_err),
           "plan_table_len": np.array(tab_len, dtype=np.int64), "plan_tables": np.concatenate(tabs)}
    case, bytes_ = [], []
    for name, has_dk, extra, width in WORKSPACES:
        fn = getattr(lib, name)
        for dk in ((64, 128, 192, 83) if has_dk else (width,)):
            for h in (1, 6):
                for n in (1, 300, 1024, 1025, LONG):
                    for k in _keys(dk):
                        args = [ctypes.c_int64(n), ctypes.c_int(k), ctypes.c_int(h)] + ([ctypes.c_int(dk)] if has_dk else [])
                        case.append("%s dk=%d h=%d n=%d k=%d" % (name, dk, h, n, k))
                        bytes_.append(fn(*args, *[ctypes.c_int(e) for e in extra]))
    out["workspace_case"] = np.array(case)
    out["workspace_bytes"] = np.array(bytes_, dtype=np.uint64)
    return out


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    res = run(ctypes.CDLL(sys.argv[1]))
    np.savez_compressed(GOLDEN, **res)
    print("%d plan cases, %d workspace cases -> %s (%d bytes)" % (len(res["plan_case"]), len(res["workspace_case"]), GOLDEN,
                                                                 os.path.getsize(GOLDEN)))
