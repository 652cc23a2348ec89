"""The bf16 MFMA sparse attention at head width 192 (the reference README's MAE recipe: D = 768, h = 4, Lambda = 500), the part that
needs no GPU: the new predicates admit the recipe while every older predicate keeps its answer for dk = 192, the three switches restore
the routing of before, the workspace-size functions of the library take dk = 192, and the new kernels stay inside their scratch."""
import ctypes
import os
import sys

import pytest
import torch

from tests.attn_widths import F32_NKB4_SCRATCH, TRAIN_192 as ROW, _layer
from tests.attn_widths import stubbed_width as stubbed  # noqa: F401  (a fixture; it reads the row fixture below)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture
def row():
    return ROW


def test_dk192_predicate_of_ops():
    from snuffy_amd import ops
    for k in (1, 128, 129, 500, 1024):
        assert ops.mfma_attn_dk192_supported(k) is True, k
        assert ops.mfma_attn_dk192_supported(k, 30000, 2 * 768) is True, k
    for k in (0, 1025):
        assert ops.mfma_attn_dk192_supported(k) is False, k
    assert not ops.mfma_attn_dk192_supported(500, 0xffff01)                      # 24-bit row x pitch products
    assert not ops.mfma_attn_dk192_supported(500, 1000, 1 << 24)                 # row pitch
    assert not ops.mfma_attn_dk192_supported(500, 2_000_000, 1536)               # n * pitch past 2^31 elements
    assert ops.mfma_attn_dk192_supported(500, 1_000_000, 1536)


def test_older_predicates_keep_their_dk192_answers(stubbed):
    from snuffy_amd import functional as SF
    from snuffy_amd import ops
    SA = stubbed
    for k in (1, 128, 200, 500):
        assert not ops.mfma_attn_supported(k, 192) and not ops.mfma_attn_supported(k, 192, 3000, 1536)
        assert not ops.mfma_attn_bwd_supported(k, 192)
        assert not ops.mfma_attn_dropout_supported(k, 192)
        assert not ops.mfma_attn_train_chunks_supported(k, 192)
    assert SF.head_pad(192) is None
    for enc in (0.0, 0.1):
        layer = _layer(768, 4, 500, enc).train()
        for k in (128, 500):
            assert not SA.fused_layer0_train_ok(layer, 16384, 768, k)
            assert not SA.fused_layer0_shape_ok(layer, 16384, 768, k)
            assert not SA.fused_layer0_chunked_ok(layer, 16384, 768, k)


def test_dk192_ok_admits_the_mae_recipe(stubbed, monkeypatch):
    SA = stubbed
    from snuffy_amd import functional as SF
    assert isinstance(SF.MFMA_ATTN_DK192, bool)
    for enc in (0.0, 0.1):
        rec = _layer(768, 4, 500, enc).train()
        assert SA.fused_layer0_dk192_ok(rec, 16384, 768, 500), enc
        assert SA.fused_layer0_dk192_ok(rec, 16391, 768), enc                      # k defaults to Lambda
        assert SA.fused_layer0_dk192_ok(rec, 300, 768), enc                        # ... capped by n
        assert SA.fused_layer0_dk192_ok(rec, 16384, 768, 1) and SA.fused_layer0_dk192_ok(rec, 16384, 768, 1024)
        assert not SA.fused_layer0_dk192_ok(rec, 16384, 768, 1025)
        assert not SA.fused_layer0_dk192_ok(rec, 16384, 768, 0)
    # other head widths are not this predicate's
    assert not SA.fused_layer0_dk192_ok(_layer(768, 6, 500, 0.0).train(), 16384, 768, 500)
    assert not SA.fused_layer0_dk192_ok(_layer(384, 4, 500, 0.0).train(), 16384, 384, 500)
    assert not SA.fused_layer0_dk192_ok(_layer(768, 4, 500, 0.1, "gelu").train(), 16384, 768, 500)
    layer = _layer(768, 4, 500, 0.1).train()
    for site in (layer.sublayer[0].dropout, layer.sublayer[1].dropout, layer.feed_forward.dropout):
        site.p = 1.0                                                               # 1 / (1 - p) does not exist
        assert not SA.fused_layer0_dk192_ok(layer, 16384, 768, 500)
        site.p = 0.1
    assert SA.fused_layer0_dk192_ok(layer, 16384, 768, 500)
    layer.self_attn.linears[0].weight.requires_grad_(False)                       # a frozen parameter: the chain returns every gradient
    assert not SA.fused_layer0_dk192_ok(layer, 16384, 768, 500)
    layer.self_attn.linears[0].weight.requires_grad_(True)
    assert SA.fused_layer0_dk192_ok(layer, 16384, 768, 500)
    # the three switches
    monkeypatch.setattr(SA, "FUSED_BF16_ENCODER_DROPOUT", False)                  # encoder dropout inside the chain is a switch of its own
    assert not SA.fused_layer0_dk192_ok(layer, 16384, 768, 500)
    assert SA.fused_layer0_dk192_ok(_layer(768, 4, 500, 0.0).train(), 16384, 768, 500)
    monkeypatch.setattr(SA, "FUSED_BF16_ENCODER_DROPOUT", True)
    monkeypatch.setattr(SA, "FUSED_BF16_DK192", False)
    assert not SA.fused_layer0_dk192_ok(layer, 16384, 768, 500)
    monkeypatch.setattr(SA, "FUSED_BF16_DK192", True)
    monkeypatch.setattr(SA, "FUSED_BF16_TRAINING", False)
    assert not SA.fused_layer0_dk192_ok(layer, 16384, 768, 500)


def test_fused_layer0_ok_follows_the_dk192_predicate(stubbed, monkeypatch):
    SA = stubbed
    x = torch.zeros(3000, 768)
    for enc_drop, train in ((0.0, True), (0.1, True), (0.1, False)):
        layer = _layer(768, 4, 500, enc_drop).train(train)
        for k in (1, 128, 129, 500, 1024, 1025):
            assert SA.fused_layer0_ok(x, torch.arange(k), layer, "bf16") == SA.fused_layer0_dk192_ok(layer, 3000, 768, k) == (k <= 1024)
        assert not SA.fused_layer0_ok(x, torch.arange(500), layer, "fp32")
        assert not SA.fused_layer0_ok(x.clone().requires_grad_(), torch.arange(500), layer, "bf16")
        assert not SA.fused_layer0_ok(x, torch.arange(0), layer, "bf16")
        monkeypatch.setattr(SA, "FUSED_BF16_DK192", False)                         # the routing of before: dk = 192 stays out
        for k in (1, 128, 500):
            assert not SA.fused_layer0_ok(x, torch.arange(k), layer, "bf16")
        monkeypatch.setattr(SA, "FUSED_BF16_DK192", True)
    # the switch is about dk = 192 only
    monkeypatch.setattr(SA, "FUSED_BF16_DK192", False)
    other = _layer(768, 6, 500, 0.1).train()
    assert SA.fused_layer0_ok(x, torch.arange(500), other, "bf16")


def test_workspace_size_functions_take_dk192():
    from snuffy_amd import _ffi
    assert os.path.exists(_ffi.LIB_PATH), "libsnuffy_hip.so missing: run __graft_entry__.build()"
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    fwd = lib.snf_sparse_attn_fwd_workspace_bytes
    fwd.restype, fwd.argtypes = ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    bwd = lib.snf_sparse_attn_bwd_mfma_chunked_workspace_bytes
    bwd.restype, bwd.argtypes = ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    from snuffy_amd import ops
    for n in (1, 3000, 30000):
        assert fwd(n, 500, 4, 192, 1) > 0
        assert fwd(n, 1025, 4, 192, 1) == 0
        # four chunks of 125 keys: the statistics of every chunk ride behind the partial tiles
        assert fwd(n, 500, 4, 192, 1) >= 4 * 4 * n * 2 * 4
        for dt in (ops.DT_F32, ops.DT_BF16):
            assert bwd(n, 500, 4, 192, dt) > 0
            assert bwd(n, 100, 4, 192, dt) > 0                                     # one chunk still runs the chunked kernel at dk = 192
            assert bwd(n, 1025, 4, 192, dt) == 0
        assert bwd(n, 500, 4, 192, ops.DT_BF16) >= bwd(n, 500, 4, 192, ops.DT_F32) + 2 * n * 768 * 4
    # the other widths keep their sizes' rules: one chunk needs no workspace there
    assert bwd(3000, 224, 2, 128, ops.DT_F32) == 0 and bwd(3000, 225, 2, 128, ops.DT_F32) > 0
    assert fwd(3000, 8 * 224 + 1, 2, 128, 1) == 0 and fwd(3000, 500, 4, 96, 1) == 0


def test_dk192_kernels_keep_their_scratch():
    """The dk = 192 forward, statistics and backward-over-chunks kernels spill nothing, except the f32-operand forward at 4 key blocks,
    which is held to the bytes measured when it was added (F32_NKB4_SCRATCH above says why)."""
    import scan_spills
    objdir = os.path.join(scan_spills.ROOT, "snuffy_amd", "build")
    if not os.path.isdir(objdir) or not os.path.exists(os.path.join(objdir, "sparse_attn_mfma_dk192.o")):
        pytest.skip("no build objects here (the library was built elsewhere)")
    try:
        ks = scan_spills.kernels(objdir)
    except RuntimeError as exc:
        pytest.skip(str(exc))
    names = scan_spills.demangle([k[1] for k in ks])
    mine = {name: scratch for (_, _, scratch, _, _), name in zip(ks, names)
            if any(t in name for t in ("sparse_attn_mfma_kernel<192,", "sparse_attn_stats_kernel<192,", "sparse_attn_bwd_chunk_kernel<192,"))}
    fwd = [n for n in mine if "sparse_attn_mfma_kernel<192," in n]
    assert len(fwd) == 20, sorted(mine)                 # {1, 2, 4} blocks + chunked {2, 4}, x 2 operand types x with / without A | lse
    assert sum("sparse_attn_stats_kernel<192," in n for n in mine) == 4
    assert sum("sparse_attn_bwd_chunk_kernel<192," in n for n in mine) == 5
    bad = {}
    for name, scratch in mine.items():
        allowed = 0
        if "sparse_attn_mfma_kernel<192, 4, float, " in name:
            allowed = F32_NKB4_SCRATCH["<192, 4, float, true" in name]
        if scratch > allowed:
            bad[name] = scratch
    assert not bad, bad
