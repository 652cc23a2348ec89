"""The fused bf16 training chain above one key chunk and at padded head widths, the part that needs no GPU: fused_layer0_chunked_ok
admits the reference's recipes (Lambda = 500 / 900, h = 4 at D = 384 / 512) while the older predicates keep their answers, the switch
FUSED_BF16_KEY_CHUNKS restores the routing of before, and the new C entry points are declared, exported and in the ctypes table."""
import ctypes
import os
import re

import torch

from tests.attn_widths import _layer, stubbed  # noqa: F401  (stubbed is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "snuffy_hip.h")

NEW = {"snf_sparse_attn_bwd_mfma_chunked": 26, "snf_sparse_attn_bwd_mfma_chunked_workspace_bytes": 5}


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
    # the arguments of snf_sparse_attn_bwd_mfma_ex with (workspace, workspace_bytes) in front of the stream
    ex, ch = _ffi.SIGNATURES["snf_sparse_attn_bwd_mfma_ex"][1], _ffi.SIGNATURES["snf_sparse_attn_bwd_mfma_chunked"][1]
    assert ch == ex[:-1] + [ctypes.c_void_p, ctypes.c_size_t] + ex[-1:]
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert "`%s`" % name in text, "%s is missing from INTEGRATION.md" % name


def test_chunk_predicate_of_ops():
    from snuffy_amd import ops
    for k, dk, want in ((1, 128, True), (225, 128, True), (8 * 224, 128, True), (8 * 224 + 1, 128, False), (8 * 256, 64, True),
                        (8 * 256 + 1, 64, False), (500, 96, False), (500, 192, False), (0, 64, False)):
        assert ops.mfma_attn_train_chunks_supported(k, dk) is want, (k, dk)
    # the one-chunk predicates keep their answers
    assert ops.mfma_attn_bwd_supported(224, 128) and not ops.mfma_attn_bwd_supported(225, 128)
    assert ops.mfma_attn_dropout_supported(256, 64) and not ops.mfma_attn_dropout_supported(257, 64)


def test_chunked_ok_admits_the_recipes_and_the_older_predicates_keep_their_answers(stubbed, monkeypatch):
    SA = stubbed
    assert SA.FUSED_BF16_KEY_CHUNKS is True
    layer = _layer(768, 6, 200, 0.1).train()
    assert SA.fused_layer0_chunked_ok(layer, 16384, 768, 225)
    assert not SA.fused_layer0_train_ok(layer, 16384, 768, 225) and not SA.fused_layer0_train_ok(layer, 16384, 768, 300)
    assert not SA.fused_layer0_shape_ok(layer, 16384, 768, 225) and not SA.fused_layer0_shape_ok(layer, 16384, 768, 300)
    assert SA.fused_layer0_chunked_ok(layer, 16384, 768, 8 * 224) and not SA.fused_layer0_chunked_ok(layer, 16384, 768, 8 * 224 + 1)
    for d, lam in ((512, 900), (384, 500), (384, 900)):                   # h = 4: dk = 128, and dk = 96 riding padded to 128
        for enc in (0.0, 0.1):
            rec = _layer(d, 4, lam, enc).train()
            assert SA.fused_layer0_chunked_ok(rec, 16384, d, lam), (d, lam, enc)
            assert SA.fused_layer0_chunked_ok(rec, 16391, d), (d, lam, enc)                # k defaults to Lambda
            assert not SA.fused_layer0_train_ok(rec, 16384, d, lam)
            assert SA.fused_layer0_ok(torch.zeros(3000, d), torch.arange(lam), rec, "bf16")
    # dk = 96 at ONE chunk is new ground too (padded); the unpadded widths at one chunk are what fused_layer0_train_ok takes already
    assert SA.fused_layer0_chunked_ok(_layer(384, 4, 200, 0.0).train(), 16384, 384, 200)
    # dk = 192 (the MAE recipe, D = 768 with h = 4) has no padded form
    assert not SA.fused_layer0_chunked_ok(_layer(768, 4, 500, 0.0).train(), 16384, 768, 500)
    assert not SA.fused_layer0_chunked_ok(_layer(768, 6, 500, 0.1, "gelu").train(), 16384, 768, 500)
    for site in (layer.sublayer[0].dropout, layer.sublayer[1].dropout, layer.feed_forward.dropout):
        site.p = 1.0                                                       # 1 / (1 - p) does not exist
        assert not SA.fused_layer0_chunked_ok(layer, 16384, 768, 500)
        site.p = 0.1
    assert SA.fused_layer0_chunked_ok(layer, 16384, 768, 500)
    monkeypatch.setattr(SA, "FUSED_BF16_ENCODER_DROPOUT", False)          # encoder dropout inside the chain is a switch of its own
    assert not SA.fused_layer0_chunked_ok(layer, 16384, 768, 500)
    assert SA.fused_layer0_chunked_ok(_layer(768, 6, 500, 0.0).train(), 16384, 768, 500)
    monkeypatch.setattr(SA, "FUSED_BF16_ENCODER_DROPOUT", True)
    layer.self_attn.linears[0].weight.requires_grad_(False)               # a frozen parameter: the chain returns every gradient
    assert not SA.fused_layer0_chunked_ok(layer, 16384, 768, 500)
    layer.self_attn.linears[0].weight.requires_grad_(True)
    monkeypatch.setattr(SA, "FUSED_BF16_KEY_CHUNKS", False)
    assert not SA.fused_layer0_chunked_ok(layer, 16384, 768, 225)
    monkeypatch.setattr(SA, "FUSED_BF16_KEY_CHUNKS", True)
    monkeypatch.setattr(SA, "FUSED_BF16_TRAINING", False)
    assert not SA.fused_layer0_chunked_ok(layer, 16384, 768, 225)


def test_the_switch_restores_the_routing_of_before(stubbed, monkeypatch):
    SA = stubbed
    x = torch.zeros(3000, 768)
    for enc_drop, train in ((0.0, True), (0.1, True), (0.1, False)):
        layer = _layer(768, 6, 500, enc_drop).train(train)
        monkeypatch.setattr(SA, "FUSED_BF16_KEY_CHUNKS", False)
        for k in (1, 200, 224, 225, 300, 500):                             # today's answers: the one-chunk predicate alone
            assert SA.fused_layer0_ok(x, torch.arange(k), layer, "bf16") == SA.fused_layer0_train_ok(layer, 3000, 768, k) == (k <= 224)
        monkeypatch.setattr(SA, "FUSED_BF16_KEY_CHUNKS", True)
        assert SA.fused_layer0_ok(x, torch.arange(500), layer, "bf16")
        assert SA.fused_layer0_ok(x, torch.arange(200), layer, "bf16")
        assert not SA.fused_layer0_ok(x, torch.arange(500), layer, "fp32")
        assert not SA.fused_layer0_ok(x.clone().requires_grad_(), torch.arange(500), layer, "bf16")
    padded = _layer(384, 4, 500, 0.1).train()
    monkeypatch.setattr(SA, "FUSED_BF16_KEY_CHUNKS", False)
    assert not SA.fused_layer0_ok(torch.zeros(3000, 384), torch.arange(200), padded, "bf16")     # dk = 96 stayed out before
    monkeypatch.setattr(SA, "FUSED_BF16_KEY_CHUNKS", True)
    assert SA.fused_layer0_ok(torch.zeros(3000, 384), torch.arange(200), padded, "bf16")
