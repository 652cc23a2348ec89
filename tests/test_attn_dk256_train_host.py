"""bf16 training at head width 256 (the SimCLR ResNet-18 recipe: D = 512, h = 2, Lambda = 900), the part that needs no GPU: the
chunks of the dropout forward's main passes, the workspace of the backward over key chunks at dk = 256, the predicates and the two
switches (FUSED_BF16_DK256, SPARSE_ATTN_FN_WIDE), and the register / scratch table of the new kernels."""
import ctypes
import os
import sys

import pytest
import torch

from tests.attn_widths import BWD_TABLE, DROP_TABLE, TRAIN_256 as ROW, _layer, _nkb
from tests.attn_widths import stubbed_width as stubbed  # noqa: F401  (a fixture; it reads the row fixture below)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KMAX, MAX_CHUNKS = 128, 8


@pytest.fixture
def row():
    return ROW


def test_main_pass_chunks_for_every_key_count():
    """The forward's chunk rule restated: ceil(k / 128) chunks of ceil(k / chunks) keys.  The dropout form keeps these chunks in its main
    passes (the kernel's P depends on which keys share a 32-key block, so chunks rounded to multiples of 4 -- the 64 / 128 / 192
    family's way -- would not reproduce the undropped P bit for bit): the size stays <= 128, the chunks cover k, k >= 129 gives >= 2
    chunks, every chunk of a chunked launch needs 2 or 4 key blocks (the counts the MODE 2 dropout kernels are built for), and chunk
    starts take every residue mod 4 (the kernel draws the two Philox groups a lane's 4 keys straddle)."""
    residues = set()
    for k in range(1, MAX_CHUNKS * KMAX + 1):
        count = -(-k // KMAX)
        assert (count >= 2) == (k >= 129) and count <= MAX_CHUNKS
        if count == 1:
            continue                                                             # one launch holds all keys: key0 = 0
        size = -(-k // count)
        assert 65 <= size <= KMAX and (count - 1) * size < k <= count * size, k  # the chunks cover k and the last one is not empty
        for c in range(count):
            kc = min(size, k - c * size)
            assert 1 <= kc <= KMAX and _nkb(kc) in (2, 4), (k, c, kc)
            residues.add((c * size) & 3)
    assert residues == {0, 1, 2, 3}


def test_main_pass_chunks_are_the_plans():
    """... and that restated rule is what the library plans at this width (the varlen plan reports the chunks; the single bag takes the
    same ones)."""
    import numpy as np
    from snuffy_amd import _ffi
    lib = _ffi.load()
    off = np.array([0, 300, 5300], dtype=np.int64)
    for k in (1, 128, 129, 257, 900, 1023, 1024):
        need, ws, nc, ck = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_int(-1), ctypes.c_int(-1)
        assert lib.snf_sparse_attn_varlen_dk256_plan(ctypes.c_void_p(off.ctypes.data), 2, k, 2, None, 0, ctypes.byref(need), ctypes.byref(ws),
                                                     ctypes.byref(nc), ctypes.byref(ck)) == 0
        assert nc.value == -(-k // KMAX) and ck.value == -(-k // nc.value), k


def test_backward_workspace_takes_dk256():
    from snuffy_amd import _ffi, ops
    assert os.path.exists(_ffi.LIB_PATH), "libsnuffy_hip.so missing: run __graft_entry__.build()"
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    bwd = lib.snf_sparse_attn_bwd_mfma_chunked_workspace_bytes
    bwd.restype, bwd.argtypes = ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    for n in (1, 3000, 32768):
        for dt in (ops.DT_F32, ops.DT_BF16):
            for k in (1, 100, 900, 1024):                                        # one chunk still runs the chunked kernel at dk = 256
                assert bwd(n, k, 2, 256, dt) > 0, (n, k, dt)
            assert bwd(n, 1025, 2, 256, dt) == 0 and bwd(n, 0, 2, 256, dt) == 0
        acc = -(-(n * 512 * 4) // 256) * 256                                     # one fp32 accumulator [n, h dk], rounded to 256 bytes
        for k in (100, 900):
            assert bwd(n, k, 2, 256, ops.DT_BF16) == bwd(n, k, 2, 256, ops.DT_F32) + 2 * acc
    # the answers tests/test_attn_dk192_host.py asserts at the other widths
    for n in (1, 3000, 30000):
        for dt in (ops.DT_F32, ops.DT_BF16):
            assert bwd(n, 500, 4, 192, dt) > 0 and bwd(n, 100, 4, 192, dt) > 0 and bwd(n, 1025, 4, 192, dt) == 0
        assert bwd(n, 500, 4, 192, ops.DT_BF16) >= bwd(n, 500, 4, 192, ops.DT_F32) + 2 * n * 768 * 4
    assert bwd(3000, 224, 2, 128, ops.DT_F32) == 0 and bwd(3000, 225, 2, 128, ops.DT_F32) > 0
    assert bwd(3000, 256, 2, 64, ops.DT_F32) == 0 and bwd(3000, 257, 2, 64, ops.DT_F32) > 0


def test_abi_has_the_dropout_entry():
    from snuffy_amd import _ffi
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    assert hasattr(lib, "snf_sparse_attn_fwd_mfma_dk256_dropout")
    res, args = _ffi.SIGNATURES["snf_sparse_attn_fwd_mfma_dk256_dropout"]
    assert res is ctypes.c_int
    assert args == _ffi.SIGNATURES["snf_sparse_attn_fwd_mfma_dk256"][1] + [ctypes.c_float, ctypes.c_uint64, ctypes.c_uint64]


def test_train_predicate_of_ops():
    from snuffy_amd import ops
    ks = (0, 1, 128, 129, 900, 1024, 1025)
    assert [ops.mfma_attn_dk256_train_supported(k) for k in ks] == [False, True, True, True, True, True, False]
    assert ops.mfma_attn_dk256_train_supported(900, 0xffff00, 128) and not ops.mfma_attn_dk256_train_supported(900, 0xffff01, 128)
    assert not ops.mfma_attn_dk256_train_supported(900, 100, 1 << 24)
    assert ops.mfma_attn_dk256_train_supported(900, 32768, 1024)
    # the older predicates keep their answers at this width
    for k in (1, 128, 200, 900):
        assert not ops.mfma_attn_supported(k, 256) and not ops.mfma_attn_bwd_supported(k, 256)
        assert not ops.mfma_attn_dropout_supported(k, 256) and not ops.mfma_attn_train_chunks_supported(k, 256)


def test_shipped_switches():
    """SPARSE_ATTN_FN_WIDE ships off (one measured row is behind the previous routing); FUSED_BF16_DK256 is a plain bool whose shipped
    value is the measurement's (profiles/attn_dk256_train.txt), so the tests here set it themselves."""
    from snuffy_amd import autograd as SA
    assert SA.SPARSE_ATTN_FN_WIDE is False
    assert isinstance(SA.FUSED_BF16_DK256, bool)


def test_dk256_ok_follows_the_key_range_and_the_switches(stubbed, monkeypatch):
    SA = stubbed
    for enc in (0.0, 0.1):
        rec = _layer(512, 2, 900, enc).train()
        assert SA.fused_layer0_dk256_ok(rec, 32768, 512, 900), enc
        assert SA.fused_layer0_dk256_ok(rec, 8000, 512) and SA.fused_layer0_dk256_ok(rec, 300, 512)   # k defaults to Lambda, capped by n
        assert SA.fused_layer0_dk256_ok(rec, 8000, 512, 1) and SA.fused_layer0_dk256_ok(rec, 8000, 512, 1024)
        assert not SA.fused_layer0_dk256_ok(rec, 8000, 512, 1025) and not SA.fused_layer0_dk256_ok(rec, 8000, 512, 0)
    assert SA.fused_layer0_dk256_ok(_layer(256, 1, 100, 0.0).train(), 8000, 256, 100)
    assert SA.fused_layer0_dk256_ok(_layer(768, 3, 500, 0.0).train(), 8000, 768, 500)
    # other head widths and activations are not this predicate's
    assert not SA.fused_layer0_dk256_ok(_layer(512, 4, 900, 0.0).train(), 8000, 512, 900)
    assert not SA.fused_layer0_dk256_ok(_layer(768, 4, 500, 0.0).train(), 8000, 768, 500)
    assert not SA.fused_layer0_dk256_ok(_layer(512, 2, 900, 0.1, "gelu").train(), 8000, 512, 900)
    layer = _layer(512, 2, 900, 0.1).train()
    for site in (layer.sublayer[0].dropout, layer.sublayer[1].dropout, layer.feed_forward.dropout):
        site.p = 1.0
        assert not SA.fused_layer0_dk256_ok(layer, 8000, 512, 900)
        site.p = 0.1
    layer.self_attn.linears[0].weight.requires_grad_(False)
    assert not SA.fused_layer0_dk256_ok(layer, 8000, 512, 900)
    layer.self_attn.linears[0].weight.requires_grad_(True)
    assert SA.fused_layer0_dk256_ok(layer, 8000, 512, 900)
    # the three switches
    monkeypatch.setattr(SA, "FUSED_BF16_ENCODER_DROPOUT", False)
    assert not SA.fused_layer0_dk256_ok(layer, 8000, 512, 900)
    assert SA.fused_layer0_dk256_ok(_layer(512, 2, 900, 0.0).train(), 8000, 512, 900)
    monkeypatch.setattr(SA, "FUSED_BF16_ENCODER_DROPOUT", True)
    monkeypatch.setattr(SA, "FUSED_BF16_DK256", False)
    assert not SA.fused_layer0_dk256_ok(layer, 8000, 512, 900)
    monkeypatch.setattr(SA, "FUSED_BF16_DK256", True)
    monkeypatch.setattr(SA, "FUSED_BF16_TRAINING", False)
    assert not SA.fused_layer0_dk256_ok(layer, 8000, 512, 900)


def test_fused_layer0_ok_at_dk256_and_elsewhere(stubbed, monkeypatch):
    SA = stubbed
    x = torch.zeros(3000, 512)
    for enc_drop, train in ((0.0, True), (0.1, True), (0.1, False)):
        layer = _layer(512, 2, 900, enc_drop).train(train)
        for k in (1, 128, 129, 900, 1024, 1025):
            assert SA.fused_layer0_ok(x, torch.arange(k), layer, "bf16") == SA.fused_layer0_dk256_ok(layer, 3000, 512, k) == (k <= 1024)
        assert not SA.fused_layer0_ok(x, torch.arange(900), layer, "fp32")
        assert not SA.fused_layer0_ok(x.clone().requires_grad_(), torch.arange(900), layer, "bf16")
        monkeypatch.setattr(SA, "FUSED_BF16_DK256", False)                         # the routing of before: dk = 256 stays out
        for k in (1, 128, 900):
            assert not SA.fused_layer0_ok(x, torch.arange(k), layer, "bf16")
        monkeypatch.setattr(SA, "FUSED_BF16_DK256", True)
    # other widths ignore the switch: dk = 128 is taken on or off, dk = 192 follows its own
    x768 = torch.zeros(3000, 768)
    for on in (True, False):
        monkeypatch.setattr(SA, "FUSED_BF16_DK256", on)
        assert SA.fused_layer0_ok(x, torch.arange(500), _layer(512, 4, 500, 0.1).train(), "bf16")
        for on192 in (True, False):
            monkeypatch.setattr(SA, "FUSED_BF16_DK192", on192)
            assert SA.fused_layer0_ok(x768, torch.arange(500), _layer(768, 4, 500, 0.1).train(), "bf16") is on192


def test_new_kernels_registers_and_scratch():
    """Every dropout-forward instantiation and the bf16-operand backward forms at DK = 256 have zero scratch; the counts of the new
    instantiations and the measured figures of the f32-operand forms are pinned."""
    import scan_spills
    objdir = os.path.join(scan_spills.ROOT, "snuffy_amd", "build")
    if not os.path.isdir(objdir) or not os.path.exists(os.path.join(objdir, "sparse_attn_mfma_dk256_drop.o")):
        pytest.skip("no build objects here (the library was built elsewhere)")
    try:
        ks = scan_spills.kernels(objdir)
    except RuntimeError as exc:
        pytest.skip(str(exc))
    names = scan_spills.demangle([k[1] for k in ks])
    drop, bwd, reduce256 = {}, {}, set()
    for (obj, _, scratch, spilled, vgpr), name in zip(ks, names):
        args = [a.strip() for a in name.split("<", 1)[1].split(">")[0].split(",")] if "<" in name else []
        if "sparse_attn_mfma_dk256_drop_kernel<" in name:
            assert obj == "sparse_attn_mfma_dk256_drop.o" and args[1] == "true" and args[3] == "false", (obj, name)
            assert scratch == 0 and spilled == 0, name
            drop[(int(args[0]), int(args[2]))] = (vgpr, scratch)
        elif "sparse_attn_bwd_chunk_kernel<256," in name:
            assert obj == "sparse_attn_bwd_mfma.o", (obj, name)
            if args[1] == "unsigned short":
                assert scratch == 0 and spilled == 0, name
            bwd[(args[1], int(args[2]), args[3] == "true")] = (vgpr, scratch)
        elif obj == "sparse_attn_mfma_dk256_drop.o" and "reduce_partials_kernel<256," in name:
            assert scratch == 0, name
            reduce256.add(int(args[1]))
        assert "sparse_attn_bwd_mfma_kernel<256," not in name                       # no single-launch backward at this width
    assert drop == DROP_TABLE
    assert bwd == BWD_TABLE
    assert reduce256 == {1, 2, 4}
