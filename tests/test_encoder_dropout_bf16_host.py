"""Encoder dropout inside the fused bf16 training chain, the part that needs no GPU: the four new C-ABI entry points are declared,
exported and in the ctypes table; fused_layer0_train_ok admits a training-mode layer with encoder dropout where the dropout-free chain
applies while fused_layer0_shape_ok keeps its results; the new kernels and the DROP instantiation of the bf16 GEMM keep their values in
registers."""
import ctypes
import os
import re
import sys

import pytest
import torch

from tests.attn_widths import _layer, stubbed  # noqa: F401  (stubbed is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "snuffy_hip.h")
sys.path.insert(0, os.path.join(ROOT, "tools"))

NEW = {"snf_gemm_bf16_dropout": 17, "snf_dropout_rows_bf16": 8, "snf_residual_assemble_dropout_f32": 12, "snf_colsum_fused_dropout": 10}


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
        # the dropout triple as in snf_split_hl_colsum_dropout_f32: (float p, uint64 seed, uint64 offset)
        args = _ffi.SIGNATURES[name][1]
        i = args.index(ctypes.c_float)
        assert args[i + 1:i + 3] == [ctypes.c_uint64, ctypes.c_uint64], name
    # snf_gemm_bf16_dropout = snf_gemm_bf16's arguments with the state in front of the stream
    plain, drop = _ffi.SIGNATURES["snf_gemm_bf16"][1], _ffi.SIGNATURES["snf_gemm_bf16_dropout"][1]
    assert drop == plain[:-1] + [ctypes.c_float, ctypes.c_uint64, ctypes.c_uint64] + plain[-1:]
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert "`%s`" % name in text, "%s is missing from the INTEGRATION.md round table" % name


def test_train_ok_admits_encoder_dropout_and_shape_ok_keeps_its_results(stubbed, monkeypatch):
    SA = stubbed
    layer = _layer(768, 6, 200, 0.1).train()
    assert [layer.sublayer[0].dropout.p, layer.sublayer[1].dropout.p, layer.feed_forward.dropout.p] == [0.1, 0.1, 0.1]
    assert SA.FUSED_BF16_ENCODER_DROPOUT is True
    assert SA.fused_layer0_train_ok(layer, 16384, 768, 200)             # the feature: there is no such predicate without it
    assert SA.fused_layer0_train_ok(layer, 16391, 768)                  # bags of any length; k defaults to Lambda
    assert not SA.fused_layer0_shape_ok(layer, 16384, 768, 200)         # "the dropout-free chain": unchanged
    # fused_layer0_ok is the call site: a bf16 bag that is data
    x, sel = torch.zeros(1024, 768), torch.arange(200)
    assert SA.fused_layer0_ok(x, sel, layer, "bf16")
    assert not SA.fused_layer0_ok(x, sel, layer, "fp32")
    assert not SA.fused_layer0_ok(x.clone().requires_grad_(), sel, layer, "bf16")
    # more than one key chunk stays out, as without dropout (dk = 128: 224 keys)
    assert not SA.fused_layer0_train_ok(layer, 16384, 768, 225)
    monkeypatch.setattr(SA, "FUSED_BF16_ENCODER_DROPOUT", False)        # the switch restores the routing of before
    assert not SA.fused_layer0_train_ok(layer, 16384, 768, 200)
    assert not SA.fused_layer0_ok(x, sel, layer, "bf16")
    monkeypatch.setattr(SA, "FUSED_BF16_ENCODER_DROPOUT", True)
    for site in (layer.sublayer[0].dropout, layer.sublayer[1].dropout, layer.feed_forward.dropout):
        site.p = 1.0                                                    # 1 / (1 - p) does not exist
        assert not SA.fused_layer0_train_ok(layer, 16384, 768, 200)
        site.p = 0.1
    assert SA.fused_layer0_train_ok(layer, 16384, 768, 200)
    gelu = _layer(768, 6, 200, 0.1, "gelu").train()
    assert not SA.fused_layer0_train_ok(gelu, 16384, 768, 200)
    monkeypatch.setattr(SA, "FUSED_BF16_TRAINING", False)
    assert not SA.fused_layer0_train_ok(layer, 16384, 768, 200)


def test_routing_without_encoder_dropout_is_unchanged(stubbed, monkeypatch):
    SA = stubbed
    sel = torch.arange(200)
    for enc_drop, train in ((0.0, True), (0.0, False), (0.1, False)):      # eval mode: the dropouts are off whatever their p
        layer = _layer(768, 6, 200, enc_drop).train(train)
        seen = []
        for switch in (True, False):
            monkeypatch.setattr(SA, "FUSED_BF16_ENCODER_DROPOUT", switch)
            seen.append((SA.fused_layer0_shape_ok(layer, 16384, 768, 200), SA.fused_layer0_train_ok(layer, 16384, 768, 200),
                         SA.fused_layer0_ok(torch.zeros(3000, 768), sel, layer, "bf16"), SA.fused_layer0_train_ok(layer, 16384, 768, 300),
                         SA._encoder_dropout_ps(layer)))
        assert seen[0] == seen[1] == (True, True, True, False, (0.0, 0.0, 0.0))
    # one site alone is enough to need the new path
    monkeypatch.setattr(SA, "FUSED_BF16_ENCODER_DROPOUT", True)
    layer = _layer(768, 6, 200, 0.0).train()
    layer.feed_forward.dropout.p = 0.2
    assert SA._encoder_dropout_ps(layer) == (0.0, 0.2, 0.0)
    assert SA.fused_layer0_train_ok(layer, 16384, 768, 200) and not SA.fused_layer0_shape_ok(layer, 16384, 768, 200)


def test_dropout_kernel_shapes():
    from snuffy_amd import ops
    assert ops.bf16_encoder_dropout_supported(32768, 768, 3072) and ops.bf16_encoder_dropout_supported(700, 256, 1024)
    assert ops.bf16_encoder_dropout_supported(16391, 384, 1536)
    assert not ops.bf16_encoder_dropout_supported(1024, 8200, 32800)      # the column-sum pass over dz stops at 8192 columns
    assert not ops.bf16_encoder_dropout_supported(1024, 100, 400)         # 8 bf16 per lane


def test_bf16_encoder_dropout_kernels_do_not_spill():
    """The three row passes and gemm_bf16_kernel<NI, RELU, bf16, 0, MI, DROP = true> (256- and 128-wide tiles) keep every value in
    registers, as tests/test_build_no_spills.py asks of gemm_bf16_kernel; the DROP instantiations are exactly those two."""
    import scan_spills
    objdir = os.path.join(scan_spills.ROOT, "snuffy_amd", "build")
    if not os.path.isdir(objdir) or not os.path.exists(os.path.join(objdir, "gemm.o")):
        pytest.skip("no build objects here (the library was built elsewhere)")
    try:
        ks = scan_spills.kernels(objdir)
    except RuntimeError as exc:
        pytest.skip(str(exc))
    names = scan_spills.demangle([k[1] for k in ks])
    found = {}
    for (_, _, scratch, spilled, _), n in zip(ks, names):
        for stem in ("gemm_bf16_kernel", "dropout_rows_bf16_kernel", "residual_assemble_dropout_kernel", "colsum_fused_dropout_kernel"):
            if "::" + stem in n:
                targs = n.split(stem)[1].split("(")[0]
                if stem == "gemm_bf16_kernel" and not (targs.count(",") == 5 and targs.endswith(", true>")):
                    continue
                found.setdefault(stem, {})[targs] = (scratch, spilled)
    assert sorted(found.get("gemm_bf16_kernel", {})) == ["<4, 0, 0, 0, 4, true>", "<4, 0, 0, 0, 8, true>"], found
    assert len(found.get("dropout_rows_bf16_kernel", {})) == 1 and len(found.get("residual_assemble_dropout_kernel", {})) == 2, found
    assert len(found.get("colsum_fused_dropout_kernel", {})) == 6, found
    assert all(v == (0, 0) for group in found.values() for v in group.values()), found
