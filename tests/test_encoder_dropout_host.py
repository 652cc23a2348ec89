"""Encoder dropout inside the fused fp32-class training chain, the part that needs no GPU: the three new C-ABI entry points are
declared, exported and in the ctypes table; the routing predicate takes a training-mode layer with encoder dropout on exactly where
the one-pass (hl) chain applies; the new kernels keep their values in registers."""
import ctypes
import os
import re
import sys

import pytest
import torch

from tests.attn_widths import _layer
from tests.attn_widths import stubbed_x3 as stubbed  # noqa: F401  (a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "snuffy_hip.h")
sys.path.insert(0, os.path.join(ROOT, "tools"))

NEW = {"snf_gemm_hl_dropout_bf16": 18, "snf_gemm_hl_ws_dropout_bf16": 20, "snf_split_hl_colsum_dropout_f32": 13}


def test_new_entry_points_header_ctypes_and_exports_agree():
    from snuffy_amd import _ffi
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert os.path.exists(_ffi.LIB_PATH), "libsnuffy_hip.so missing: run __graft_entry__.build()"
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name, nargs in NEW.items():
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
        assert m, "%s is not declared in include/snuffy_hip.h" % name
        assert len(m.group(1).split(",")) == nargs, name
        assert name in _ffi.SIGNATURES and len(_ffi.SIGNATURES[name][1]) == nargs, name
        assert hasattr(lib, name), "the library does not export %s" % name
    # the dropout triple sits where the attention entry points have it: (float p, uint64 seed, uint64 offset)
    for name in NEW:
        args = _ffi.SIGNATURES[name][1]
        i = args.index(ctypes.c_float)
        assert args[i + 1:i + 3] == [ctypes.c_uint64, ctypes.c_uint64], name


def test_fused_chain_takes_encoder_dropout_where_the_one_pass_chain_applies(stubbed, monkeypatch):
    SA = stubbed
    layer = _layer(768, 6, 200, 0.1).train()
    assert [layer.sublayer[0].dropout.p, layer.sublayer[1].dropout.p, layer.feed_forward.dropout.p] == [0.1, 0.1, 0.1]
    sel = torch.arange(200)
    big, small = torch.zeros(16384, 768), torch.zeros(3000, 768)
    assert SA._x3_train_hl_ok(16384, 768, 3072) and not SA._x3_train_hl_ok(3000, 768, 3072)
    assert SA.FUSED_X3_ENCODER_DROPOUT is True
    assert SA.fused_layer0_x3_ok(big, sel, layer, "fp32")               # the feature: this is False without it
    assert SA.fused_layer0_x3_ok(torch.zeros(16391, 768), sel, layer, "fp32")   # bags of any length, as the chain itself
    assert not SA.fused_layer0_x3_ok(small, sel, layer, "fp32")         # below the one-pass chain's shapes: generic chain, as before
    assert not SA.fused_layer0_x3_ok(big, sel, layer, "bf16")
    monkeypatch.setattr(SA, "X3_TRAIN_HL", False)                       # the concatenated-K branch keeps declining
    assert not SA.fused_layer0_x3_ok(big, sel, layer, "fp32")
    monkeypatch.setattr(SA, "X3_TRAIN_HL", True)
    monkeypatch.setattr(SA, "FUSED_X3_ENCODER_DROPOUT", False)          # the switch restores the routing of before
    assert not SA.fused_layer0_x3_ok(big, sel, layer, "fp32")
    # the bf16 chain declines encoder dropout, as before
    assert not SA.fused_layer0_shape_ok(layer, 16384, 768, 200)


def test_routing_without_encoder_dropout_is_unchanged(stubbed, monkeypatch):
    SA = stubbed
    sel = torch.arange(200)
    for enc_drop, train in ((0.0, True), (0.0, False), (0.1, False)):      # eval mode: the dropouts are off whatever their p
        layer = _layer(768, 6, 200, enc_drop).train(train)
        for switch in (True, False):
            monkeypatch.setattr(SA, "FUSED_X3_ENCODER_DROPOUT", switch)
            assert SA.fused_layer0_x3_ok(torch.zeros(16384, 768), sel, layer, "fp32")
            assert SA.fused_layer0_x3_ok(torch.zeros(3000, 768), sel, layer, "fp32")      # concatenated-K chain
    # one site alone is enough to need the new path
    monkeypatch.setattr(SA, "FUSED_X3_ENCODER_DROPOUT", True)
    layer = _layer(768, 6, 200, 0.0).train()
    layer.feed_forward.dropout.p = 0.2
    assert SA.fused_layer0_x3_ok(torch.zeros(16384, 768), sel, layer, "fp32")
    assert not SA.fused_layer0_x3_ok(torch.zeros(3000, 768), sel, layer, "fp32")
    assert SA._encoder_dropout_ps(layer) == (0.0, 0.2, 0.0)


def test_encoder_dropout_kernels_do_not_spill():
    """gemm_hl_kernel<ACT, OUT, SPLIT, GATE, DROP = true> is held to the bound of the other gemm_hl_kernel instantiations
    (tests/test_build_no_spills.py: <= 24 bytes, read once per tile in the epilogue), the column-sum pass to zero; the instantiations are
    exactly the two forms and their split-K twins."""
    import scan_spills
    objdir = os.path.join(scan_spills.ROOT, "snuffy_amd", "build")
    if not os.path.isdir(objdir) or not os.path.exists(os.path.join(objdir, "gemm.o")):
        pytest.skip("no build objects here (the library was built elsewhere)")
    try:
        ks = scan_spills.kernels(objdir)
    except RuntimeError as exc:
        pytest.skip(str(exc))
    names = scan_spills.demangle([k[1] for k in ks])
    gemm = {n.split("gemm_hl_kernel")[1].split("(")[0]: s for (_, _, s, _, _), n in zip(ks, names)
            if "gemm_hl_kernel<" in n and n.split("gemm_hl_kernel")[1].split("(")[0].endswith(", true>")
            and n.split("gemm_hl_kernel")[1].split("(")[0].count(",") == 4}
    cols = {n.split("split_hl_colsum_dropout_kernel")[1].split("(")[0]: s for (_, _, s, _, _), n in zip(ks, names)
            if "split_hl_colsum_dropout_kernel<" in n}
    assert len(gemm) == 4 and len(cols) == 3, (gemm, cols)
    assert all(s <= 24 for s in gemm.values()), gemm
    assert all(s == 0 for s in cols.values()), cols
