"""The native head widths of the sparse attention (192 and 256, fp32-class and bf16), as the tests see them: one record per width form
in a table, and the helpers and fixtures the width tests -- and the older packed / varlen / sampler tests -- share.  A record carries
what the forms differ in as literal values: the ops callables and predicates by name (with the route a form replaces, which the routing
tests spy on), C entry-point names, geometry constants, the recipe, switch names with their shipped values, shape lists, seeds,
tolerances and the scratch / register tables.  The host tests of the inference forms are written once over the table
(test_attn_widths_host.py lists the rows each test runs over).  The GPU files and the training host files are still one per form: each
names its record as ROW, reads every constant, name and tolerance from it, provides it to the fixtures below as its `row` fixture, and
takes every shared helper from here.  A new width form is one more record plus whatever tests are its own.

Tolerances are literals, never computed from dk.  Anything cached across tests is keyed on the row as well as the shape."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests.helpers import DEV, _ops, build_amd_milnet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))                                 # scan_spills

VL_DESC = 12
SEED, OFFSET = 1234567, 99                                                      # the device sampler's record in the model-level tests
K1 = 128                                          # keys of one launch
LENGTHS = [None, 777, 1024, 1025, 4100]           # None: exactly k rows; a row-tile tail, the last directly stored length; reduced bags


def _row(**kw):
    return types.SimpleNamespace(**kw)


# ---- scratch / register tables (tools/scan_spills.py on the build that added the kernels; DESIGN section 4 lists them) -----------------
# Scratch bytes per lane of sparse_attn_x3_dk192_kernel<NKB, AUX, MODE, VL>, with the spilled-register counts in DESIGN, which also says
# where the spilled values are read.
X3W_SCRATCH = {
    # (nkb, aux, mode, varlen): bytes.  One launch (MODE 0), single bag and varlen:
    (1, False, 0, False): 0, (1, True, 0, False): 0, (2, False, 0, False): 20, (2, True, 0, False): 32,
    (4, False, 0, False): 80, (4, True, 0, False): 92,
    (1, False, 0, True): 0, (1, True, 0, True): 0, (2, False, 0, True): 28, (2, True, 0, True): 36,
    (4, False, 0, True): 156, (4, True, 0, True): 160,
    # statistics pass of a key chunk (MODE 1)
    (2, False, 1, False): 0, (4, False, 1, False): 0, (2, False, 1, True): 0, (4, False, 1, True): 0,
    # main pass of a key chunk (MODE 2)
    (2, False, 2, False): 24, (2, True, 2, False): 32, (4, False, 2, False): 76, (4, True, 2, False): 88,
    (2, False, 2, True): 28, (2, True, 2, True): 36, (4, False, 2, True): 156, (4, True, 2, True): 152,
}
# sparse_attn_x3_dk256_kernel<NKB, AUX, MODE, VL>.  Only the varlen forms at 4 key blocks spill: they hold 128 accumulators and the 128
# Kp registers next to the bag's descriptor words.
X3Y_SCRATCH = {
    (1, False, 0, False): 0, (1, True, 0, False): 0, (2, False, 0, False): 0, (2, True, 0, False): 0,
    (4, False, 0, False): 0, (4, True, 0, False): 0,
    (1, False, 0, True): 0, (1, True, 0, True): 0, (2, False, 0, True): 0, (2, True, 0, True): 0,
    (4, False, 0, True): 72, (4, True, 0, True): 84,
    (2, False, 1, False): 0, (4, False, 1, False): 0, (2, False, 1, True): 0, (4, False, 1, True): 0,
    (2, False, 2, False): 0, (2, True, 2, False): 0, (4, False, 2, False): 0, (4, True, 2, False): 0,
    (2, False, 2, True): 0, (2, True, 2, True): 0, (4, False, 2, True): 72, (4, True, 2, True): 84,
}
# (VGPRs, scratch bytes per lane) of sparse_attn_mfma_dk256_kernel<NKB, AUX, MODE, VL>.  No form spills, the varlen forms included: at
# bf16 the Kp fragments of a key block are 64 registers, half the fp32-class figure.
A256_TABLE = {
    (1, False, 0, False): (228, 0), (1, True, 0, False): (232, 0), (2, False, 0, False): (288, 0), (2, True, 0, False): (292, 0),
    (4, False, 0, False): (420, 0), (4, True, 0, False): (420, 0),
    (1, False, 0, True): (240, 0), (1, True, 0, True): (244, 0), (2, False, 0, True): (308, 0), (2, True, 0, True): (308, 0),
    (4, False, 0, True): (436, 0), (4, True, 0, True): (436, 0),
    (2, False, 1, False): (144, 0), (4, False, 1, False): (144, 0), (2, False, 1, True): (144, 0), (4, False, 1, True): (144, 0),
    (2, False, 2, False): (288, 0), (2, True, 2, False): (292, 0), (4, False, 2, False): (416, 0), (4, True, 2, False): (420, 0),
    (2, False, 2, True): (308, 0), (2, True, 2, True): (308, 0), (4, False, 2, True): (436, 0), (4, True, 2, True): (436, 0),
}
# sparse_attn_mfma_vl192_kernel<192, NKB, unsigned short, AUX, EXT, 8, VL = true> -- (nkb, aux, ext) -- and
# sparse_attn_stats_vl192_kernel<192, NKB, unsigned short, VL = true>.  Nothing spills but the key-chunked forward at 4 key blocks with
# A | lse: one register, saved in the prologue and read back on the once-per-head Kp commit of the pooling waves.
MFMA_SCRATCH = {(1, False, False): 0, (1, True, False): 0, (2, False, False): 0, (2, True, False): 0, (4, False, False): 0,
                (4, True, False): 0, (2, False, True): 0, (2, True, True): 0, (4, False, True): 0, (4, True, True): 8}
STATS_SCRATCH = {2: 0, 4: 0}


# Scratch the single-bag dk = 192 kernels may use.  Everything on the model's path -- bf16 Q | V operands, every key-block count, the
# statistics pass, the backward over chunks -- spills nothing.  The f32-operand forward at 4 key blocks does: a pooling wave keeps 12
# V-row loads of 8 floats in flight (96 registers, converted to bf16 only on arrival) next to its 96 accumulator registers, which does
# not fit the 256 registers of two waves per SIMD; the spill code sits around the once-per-tile V publish, not inside the MFMA loops.
# Measured: 92 bytes with the attention / lse outputs, 108 without.
F32_NKB4_SCRATCH = {True: 92, False: 108}
# (VGPRs, scratch) of sparse_attn_mfma_dk256_drop_kernel<NKB, true, MODE, false>: the Philox state and the mask cost 4 - 20 registers
# over the forms without dropout.
DROP_TABLE = {(1, 0): (252, 0), (2, 0): (296, 0), (4, 0): (432, 0), (2, 2): (312, 0), (4, 2): (440, 0)}
# sparse_attn_bwd_chunk_kernel<256, QT, SERIES, FAST>.  The bf16-operand forms (the model's) spill nothing.  Series B with f32 operands
# does: its Q and V fragments are loaded as fp32 (twice the registers in flight until they are converted) next to 128 accumulator
# registers.  It is held to the 368 bytes measured on the build that added it (the model passes bf16 operands; the f32-operand forms
# serve fp32 callers and the tests' dS checks).
BWD_TABLE = {("float", 0, False): (466, 0), ("float", 1, False): (512, 368), ("unsigned short", 0, False): (437, 0),
             ("unsigned short", 1, False): (478, 0), ("unsigned short", 1, True): (475, 0)}


# ---- the table ---------------------------------------------------------------------------------------------------------------------------
# Inference forms.  Tolerances: Y_TOL / A_TOL bound logits and A of the model-level comparisons (Y_REL: the logit bound is relative above
# 1), ROWSUM the row sums of A, O_FP64 the varlen output against fp64 up to 256 keys and above.
X3_192 = _row(
    id="x3-192", family="x3", dk=192, D_K=384, H_K=2,                           # D_K: the smallest model width with dk = 192
    single="sparse_attn_fwd_x3_dk192", single_takes_n=False, varlen="sparse_attn_fwd_x3_varlen", replaced="sparse_attn_fwd_x3u",
    single_supported="x3_attn_dk192_supported", varlen_supported="varlen_attn_x3_dk192_supported", kind="fp32",
    plan_fn="snf_sparse_attn_x3_varlen_dk192_plan", ws_fn="snf_sparse_attn_fwd_x3_dk192_workspace_bytes",
    KMAX=128, MAX_CHUNKS=8, ROWS=64, NCB=6, CHUNK_MULTIPLE=4, H_PLAN=4, CK_129=68, RECIPE_CHUNKS=(4, 128),
    D=768, H=4, LAM=500, R=0.5, ACT="relu", K_TOP=250, SIZES=[500, 777, 1025, 2100, 3000],
    single_switch="X3_ATTN_DK192", pack_switch="PACK_X3_DK192", pack_ok="x3_dk192_ok", SHIPPED=(False, False),
    PRED_KS=(0, 1, 128, 129, 1024, 1025), PRED_WANT=[False, True, True, True, True, False], OK_SHAPES=((384, 2, 1), (768, 4, 1024)),
    H_OTHER=6,
    # (n, k, h) of the single-bag kernel test, seeded with n * 3 + k + dk
    SHAPES=[(1, 1, 2),
            (40, 20, 2),         # 1 key block, key tail
            (777, 64, 2),        # 2 key blocks, row-tile tail
            (1000, 100, 2),      # 4 key blocks, key tail
            (333, 128, 2),       # a full launch
            (4100, 129, 2),      # two chunks (68: 4 blocks, 61: 2 blocks), several workgroups per head
            (2000, 500, 2),      # the recipe: 128, 128, 128, 116 keys
            (333, 1024, 2)],     # 8 full chunks
    seed=lambda n, k, h: n * 3 + k + 192,
    KEYS=[20, 64, 100, 128, 129, 500, 1024], O_FP64=(2e-5, 4e-5),
    Y_TOL=1e-3, Y_REL=False, A_TOL=1e-3, ROWSUM=1e-5, ORACLE_TOL=1e-3,         # TOL["fp32"] of tests/helpers.py
    ORACLE_SIZES=[600, 1100], MIX_SIZES=[777, 300, 1025, 500], GRAPH_SIZES=[600, 1500, 900], OFF_SIZES=[600, 1100, 2048],
    kernel="sparse_attn_x3_dk192_kernel<", obj="sparse_attn_x3_dk192", TABLE=X3W_SCRATCH, reduce="x3_reduce_kernel<192,",
    absent=("sparse_attn_x3_kernel<192,",),                                     # the 64 / 128 family stays without the width
)
X3_256 = _row(
    id="x3-256", family="x3", dk=256, D_K=512, H_K=2,                           # D_K: the model width of the recipe
    single="sparse_attn_fwd_x3_dk256", single_takes_n=False, varlen="sparse_attn_fwd_x3_varlen", replaced="sparse_attn_fwd_x3u",
    single_supported="x3_attn_dk256_supported", varlen_supported="varlen_attn_x3_dk256_supported", kind="fp32",
    plan_fn="snf_sparse_attn_x3_varlen_dk256_plan", ws_fn="snf_sparse_attn_fwd_x3_dk256_workspace_bytes",
    KMAX=128, MAX_CHUNKS=8, ROWS=32, NCB=8, CHUNK_MULTIPLE=4, H_PLAN=2, CK_129=68, RECIPE_CHUNKS=(8, 116),
    D=512, H=2, LAM=900, R=7 / 9, ACT="gelu", K_TOP=200, SIZES=[900, 1100, 1500, 2100, 3000],
    single_switch="X3_ATTN_DK256", pack_switch="PACK_X3_DK256", pack_ok="x3_dk256_ok", SHIPPED=(False, True),
    PRED_KS=(0, 1, 128, 129, 900, 1024, 1025), PRED_WANT=[False, True, True, True, True, True, False],
    OK_SHAPES=((256, 1, 1), (768, 3, 1024)), H_OTHER=4,
    # (n, k, h), seeded with n * 3 + k + dk + h
    SHAPES=[(1, 1, 2),
            (40, 20, 2),         # 1 key block, key tail
            (777, 64, 2),        # 2 key blocks, row-tile tail (777 = 24 x 32 + 9)
            (1000, 100, 2),      # 4 key blocks, key tail
            (333, 128, 2),       # a full launch
            (4100, 129, 2),      # two chunks (68: 4 blocks, 61: 2 blocks), several workgroups per head
            (2000, 900, 2),      # the recipe: 7 chunks of 116 keys and one of 88
            (333, 1024, 2),      # 8 full chunks
            (500, 200, 1),       # the head loop: one head (D = 256) ...
            (500, 200, 3)],      # ... and three (D = 768)
    seed=lambda n, k, h: n * 3 + k + 256 + h,
    KEYS=[20, 64, 100, 128, 129, 900, 1024], O_FP64=(2e-5, 4e-5),
    Y_TOL=1e-3, Y_REL=False, A_TOL=1e-3, ROWSUM=1e-5, ORACLE_TOL=1e-3,
    ORACLE_SIZES=[1000, 1300], MIX_SIZES=[1100, 600, 1500, 900], SHIPPED_SIZES=[1000, 1100, 2048],
    kernel="sparse_attn_x3_dk256_kernel<", obj="sparse_attn_x3_dk256", TABLE=X3Y_SCRATCH, reduce="x3_reduce_kernel<256,",
    absent=("sparse_attn_x3_kernel<256,",),
)
MFMA_256 = _row(
    id="mfma-256", family="mfma", dk=256, D_K=512, H_K=2,
    single="sparse_attn_fwd_mfma_dk256", single_takes_n=False, varlen="sparse_attn_fwd_mfma_varlen", replaced="sparse_attn_fwd",
    single_supported="mfma_attn_dk256_supported", varlen_supported="varlen_attn_dk256_supported", kind="bf16",
    plan_fn="snf_sparse_attn_varlen_dk256_plan", ws_fn="snf_sparse_attn_fwd_mfma_dk256_workspace_bytes",
    KMAX=128, MAX_CHUNKS=8, ROWS=32, NCB=8, CHUNK_MULTIPLE=1, H_PLAN=2, CK_129=65, RECIPE_CHUNKS=(8, 113),
    D=512, H=2, LAM=900, R=7 / 9, ACT="gelu", K_TOP=200, SIZES=[900, 1100, 1500, 2100, 3000],
    single_switch="MFMA_ATTN_DK256", pack_switch="PACK_DK256", pack_ok="dk256_ok", SHIPPED=(False, True),
    PRED_KS=(0, 1, 128, 129, 900, 1024, 1025), PRED_WANT=[False, True, True, True, True, True, False],
    OK_SHAPES=((256, 1, 1), (768, 3, 1024)), H_OTHER=4,
    # (n, k, h) of test_forward (bf16 Q | V only), seeded with n * 3 + k
    SHAPES=[(1, 1, 2),
            (40, 20, 2),          # one key block, key tail
            (777, 64, 2),         # two key blocks, row-tile tail (777 = 24 x 32 + 9)
            (1000, 100, 2),       # four key blocks, key tail in the last
            (333, K1, 2),         # exactly one full launch
            (4100, K1 + 1, 2),    # two chunks (65: 4 blocks, 64: 2 blocks), several workgroups per head
            (2000, 900, 2),       # the recipe: 7 chunks of 113 keys and one of 109
            (333, 1024, 2),       # the maximum: 8 full chunks
            (500, 200, 1),        # the head loop: one head (D = 256) ...
            (500, 200, 3),        # ... and three (D = 768)
            (40000, 200, 2)],     # more row tiles than compute units: workgroups straddle heads
    KEYS=[20, 64, 100, K1, K1 + 1, 900, 1024], O_FP64=(1e-2, 1e-2),
    # the bf16 figures of the 192 packed tests: logits 2e-2 (relative above 1), A 2e-2, row sums of A 1e-3
    Y_TOL=2e-2, Y_REL=True, A_TOL=2e-2, ROWSUM=1e-3, ORACLE_TOL=1e-2,          # ORACLE_TOL: TOL["bf16"] of tests/helpers.py
    ORACLE_SIZES=[1000, 1300], MIX_SIZES=[1100, 600, 1500, 900], GRAPH_SIZES=[900, 1500, 1100], OFF_SIZES=[1000, 1100, 2048],
    SHIPPED_SIZES=[1000, 1100, 2048],
    kernel="sparse_attn_mfma_dk256_kernel<", obj="sparse_attn_mfma_dk256", TABLE=A256_TABLE, reduce="reduce_partials_kernel<256,",
    absent=("sparse_attn_mfma_kernel<256,", "sparse_attn_stats_kernel<256,"),   # the older template stays without the width
)
VARLEN_192 = _row(
    id="varlen-192", family="mfma", dk=192, D_K=384, H_K=2,
    single="sparse_attn_fwd_mfma", single_takes_n=True, varlen="sparse_attn_fwd_mfma_varlen",
    varlen_supported="varlen_attn_dk192_supported", kind="bf16",
    plan_fn="snf_sparse_attn_varlen_dk192_plan", ws_fn=None,
    KMAX=128, MAX_CHUNKS=8, NCB=6, CHUNK_MULTIPLE=1, H_PLAN=4, CK_129=65,
    D=768, H=4, LAM=500, R=0.5, ACT="relu", K_TOP=250, SIZES=[500, 777, 1025, 2100, 3000],
    single_switch="MFMA_ATTN_DK192", pack_switch="PACK_DK192", pack_ok="dk192_ok",
    PRED_KS=(0, 1, 128, 129, 1024, 1025), PRED_WANT=[False, True, True, True, True, False], OK_SHAPES=((384, 2, 1), (768, 4, 1024)),
    H_OTHER=6,
    KEYS=[20,                                       # 1 key block
          64,                                       # 2 key blocks
          100,                                      # 4 key blocks with a key tail
          128,                                      # a full launch
          129,                                      # two chunks whose key-block counts differ (65: 4, 64: 2)
          500,                                      # the recipe: 4 x 125
          1024],                                    # 8 full chunks
    O_FP64=(1e-2, 1e-2),
    # the bf16 figures of test_gpu_varlen_chunks.py: logits 2e-2 (relative above 1), A 2e-2, row sums of A 1e-3
    Y_TOL=2e-2, Y_REL=True, A_TOL=2e-2, ROWSUM=1e-3,
    ORACLE_SIZES=[600, 1100], MIX_SIZES=[777, 150, 1025, 500], GRAPH_SIZES=[600, 1500, 900], OFF_SIZES=[600, 1100, 2048],
)
# Training forms (bf16).  SHAPES are (n, k, h) of the forward / backward kernel tests, BIG has more row tiles than compute units
# (workgroups straddle heads; bf16 operands only).
TRAIN_192 = _row(
    id="train-192", family="mfma", dk=192, D=768, H=4, LAM=500,
    single="sparse_attn_fwd_mfma", single_takes_n=True, single_supported="mfma_attn_dk192_supported",
    supported="mfma_attn_dk192_supported", train_switch="FUSED_BF16_DK192",
    single_switch="MFMA_ATTN_DK192",
    # smallest possible; one partly filled tile, one key block; two row tiles, 4th key block partly filled; exactly one full chunk; two
    # chunks, the second nearly empty (2 key blocks); the recipe's keys and heads; eight full chunks
    SHAPES=[(1, 1, 1), (33, 7, 2), (130, 97, 1), (777, 128, 4), (300, 129, 2), (1000, 500, 4), (257, 1024, 1)],
    BIG=(40000, 200, 4),
    DROP_SHAPES=[(130, 97, 1, "f32"), (300, 300, 2, "bf16"), (1000, 500, 4, "bf16")],
)
TRAIN_256 = _row(
    id="train-256", family="mfma", dk=256, D=512, H=2, LAM=900,
    single="sparse_attn_fwd_mfma_dk256", single_takes_n=False, supported="mfma_attn_dk256_train_supported",
    train_switch="FUSED_BF16_DK256",
    # smallest possible; one key block with a tail; two blocks, row-tile tail; four blocks, k % 4 != 0 (the scalar dS path); exactly one
    # chunk; two chunks (forward 65 + 64: the second starts at key 65, off a multiple of 4; backward 96 + 33); the recipe's keys
    # (forward 7 chunks of 113 and one of 109, starts at every residue mod 4; backward 7 x 128 + 4); eight full chunks
    SHAPES=[(1, 1, 1), (40, 20, 2), (777, 64, 2), (130, 97, 1), (333, 128, 2), (300, 129, 2), (640, 900, 2), (257, 1024, 1)],
    BIG=(40000, 200, 2),
    DROP_SHAPES=[(130, 97, 1), (300, 300, 2), (640, 900, 2)],
)
# the dropout state of the training kernel tests
P_DROP, DROP_SEED, DROP_OFFSET = 0.1, 987654321, 5


def rows(*table):
    """Parametrises a test over the given rows; the fixtures below read the row of the running case."""
    return pytest.mark.parametrize("row", table, ids=[r.id for r in table])


def op(row, field):
    """The ops callable or predicate the record names in `field`."""
    return getattr(_ops(), getattr(row, field))


def single_bag(row, q, v, kp, h, **kw):
    """The single-bag forward of the row (the older bf16 entry point, which serves dk = 192, takes the row count)."""
    if row.single_takes_n:
        return op(row, "single")(q, v, kp, q.shape[0], h, **kw)
    return op(row, "single")(q, v, kp, h, **kw)


# ---- host side: plans, key blocks, build objects -----------------------------------------------------------------------------------------
def _offsets(sizes):
    off = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum(sizes, out=off[1:])
    return off


def _plan(row, lib, sizes, k, h, table=True):
    """(rc, table, workspace bytes, chunks, keys per chunk)"""
    fn, off = getattr(lib, row.plan_fn), _offsets(sizes)
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


def nkb_of_family(fam, kc, dk):
    """Key-block count the planner of the 64 / 128 families picks for a launch of kc keys."""
    opts = (1, 2, 4, 6, 7, 8) if fam == "mfma" else (2, 4, 7, 8)
    return next(o for o in opts if 32 * o >= kc and not (o == 8 and dk == 128))


def _r256(b):
    return -(-b // 256) * 256


def built_kernels(obj):
    """[((object, symbol, scratch, spilled, vgprs), demangled name, template arguments)] of the build tree; skips where the library was
    built elsewhere."""
    import scan_spills
    objdir = os.path.join(scan_spills.ROOT, "snuffy_amd", "build")
    if not os.path.isdir(objdir) or not os.path.exists(os.path.join(objdir, obj)):
        pytest.skip("no build objects here (the library was built elsewhere)")
    try:
        ks = scan_spills.kernels(objdir)
    except RuntimeError as exc:
        pytest.skip(str(exc))
    names = scan_spills.demangle([k[1] for k in ks])
    return [(k, name, [a.strip() for a in name.split("<", 1)[1].split(">")[0].split(",")] if "<" in name else [])
            for k, name in zip(ks, names)]


class _Lib:
    @staticmethod
    def snf_device_cu_count():
        return 256


def _layer(d, h, lam, enc_drop, act="relu"):
    net = build_amd_milnet(d, h, act, lam, 0.0, 1, enc_drop=enc_drop)
    return net.b_classifier.encoder.layers[0]


def _stub_bf16(monkeypatch):
    from snuffy_amd import autograd as SA
    from snuffy_amd import ops
    monkeypatch.setattr(ops._ffi, "load", lambda: _Lib)
    monkeypatch.setattr(SA, "FUSED_BF16_TRAINING", True)
    return SA


@pytest.fixture
def stubbed(monkeypatch):
    """The bf16 training predicates without a device."""
    return _stub_bf16(monkeypatch)


@pytest.fixture
def stubbed_width(monkeypatch, row):
    """... with the training switch of the row on, whatever its shipped default.  `row` is the test's parameter or its module's fixture."""
    SA = _stub_bf16(monkeypatch)
    monkeypatch.setattr(SA, row.train_switch, True)
    return SA


@pytest.fixture
def stubbed_x3(monkeypatch):
    """The fp32-class training predicates without a device."""
    from snuffy_amd import autograd as SA
    from snuffy_amd import functional as SF
    from snuffy_amd import ops
    monkeypatch.setattr(ops._ffi, "load", lambda: _Lib)
    monkeypatch.setattr(ops, "GEMM_HL", True)
    monkeypatch.setattr(ops, "GEMM_TN", True)
    monkeypatch.setattr(SA, "X3_TRAIN_HL", True)
    monkeypatch.setattr(SA, "FUSED_X3_TRAINING", True)
    monkeypatch.setattr(SF, "FP32_GEMM", "x3")
    return SA


# ---- varlen launches ---------------------------------------------------------------------------------------------------------------------
def _packed(sizes):
    return _ops().PackedBags(sizes, DEV)


def _sizes(k, lengths=LENGTHS):
    return [k if n is None else n for n in lengths if n is None or n >= k]


_REF64 = {}


def _fp64_reference(tag, q, v, kp, h, oracle=False):
    """softmax(Q Kp^T / sqrt(dk))^T V of one bag in fp64, computed once per tag (which names the row or family as well as the shape);
    oracle: by the CPU oracle, else restated on the operands' device."""
    if tag not in _REF64:
        if oracle:
            from oracle import snuffy_oracle as orc
            _REF64[tag] = orc.sparse_attention(q.double().cpu(), kp.double().cpu(), v.double().cpu(), h)[0]
        else:
            n, d = q.shape
            k, dk = kp.shape[0], d // h
            qd = q.double().view(n, h, dk).transpose(0, 1)
            vd = v.double().view(n, h, dk).transpose(0, 1)
            kd = kp.double().view(k, h, dk).transpose(0, 1)
            p = torch.softmax(qd @ kd.transpose(1, 2) / dk ** 0.5, dim=-1)
            _REF64[tag] = (p.transpose(1, 2) @ vd).transpose(0, 1).reshape(k, d)
    return _REF64[tag]


# ---- model level -------------------------------------------------------------------------------------------------------------------------
def _bags(sizes, d, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(1, n, d, generator=g).to(DEV) for n in sizes]


def _loop(net, bags):
    out, sels = [], []
    for x in bags:
        out.append(net(x))
        sels.append([tuple(None if t is None else t.clone() for t in l.last_selection) for l in net.b_classifier.encoder.layers])
    return out, sels


def y_bound(row, y_ref):
    return row.Y_TOL * max(1.0, y_ref.abs().max().item()) if row.Y_REL else row.Y_TOL


def _close(row, ref, got, n, k=None):
    (c0, y0, a0), (c1, y1, a1) = ref, got
    assert c1.shape == c0.shape and y1.shape == y0.shape and a1.shape == a0.shape == (1, row.H, n, row.LAM if k is None else k)
    assert torch.equal(c0, c1)                           # critic scores: same kernel, row-wise
    dy, da = (y0 - y1).abs().max().item(), (a0 - a1).abs().max().item()
    ds = (a1.sum(-1) - 1).abs().max().item()
    print("n=%d: |dlogit| %.3g  |dA| %.3g  |rowsum - 1| %.3g" % (n, dy, da, ds))
    assert dy <= y_bound(row, y0), (y0, y1)
    assert da <= row.A_TOL
    assert ds <= row.ROWSUM                              # only the row sum notices a chunk normalised by the wrong statistics


def outputs_close(ref, got, precision):
    tol = 2e-5 if precision == "fp32" else 2e-2
    (c0, y0, a0), (c1, y1, a1) = ref, got
    assert c1.shape == c0.shape and y1.shape == y0.shape and a1.shape == a0.shape
    assert torch.equal(c0, c1)
    err_y, err_a = (y0 - y1).abs().max().item(), (a0 - a1).abs().max().item()
    print("logit err %.3e (|y| %.3e)  A err %.3e" % (err_y, y0.abs().max().item(), err_a))
    assert err_y <= tol * max(1.0, y0.abs().max().item())
    assert err_a <= tol


def _spy(monkeypatch, name):
    ops = _ops()
    calls, real = [], getattr(ops, name)

    def spy(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(ops, name, spy)
    return calls


def _place_sampler(net, offset):
    net.b_classifier.cfg._device_sampler = _ops().DeviceSampler(torch.device(DEV, torch.cuda.current_device()), SEED, offset)
    return net.b_classifier.cfg._device_sampler


def _offset(net):
    return int(net.b_classifier.cfg._device_sampler.state[1].item())


@pytest.fixture
def pack_on(monkeypatch, row):
    """The packed switch of the row on, whatever its shipped default.  `row` is the test's parameter or its module's fixture."""
    from snuffy_amd import packed
    monkeypatch.setattr(packed, row.pack_switch, True)


@pytest.fixture
def device_sampler_on(monkeypatch):
    from snuffy_amd import packed
    monkeypatch.setattr(packed, "PACK_DEVICE_SAMPLER", True)
