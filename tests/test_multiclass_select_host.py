"""The multiclass selector and batched route, the part that needs no GPU: the domain predicates, the routing of EncoderLayer.run (with
the selection and the layer kernels stubbed) and the scratch bytes of the new kernels in the built objects."""
import os
import sys

import pytest
import torch

from snuffy_amd import functional as SF
from snuffy_amd import ops
from snuffy_amd import snuffy_multiclass as smc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_select_predicate_domain_edges():
    ok = ops.multiclass_select_supported
    assert ok(1, 100, 2, 10) and ok(64, 1, 1, 1) and ok(1, 4096, 4096, 1)
    assert ok(1, 5000, 2, 2048) and not ok(1, 5000, 2, 2049)                       # k1 <= 2048
    assert ok(1, 5000, 1, 2048) and not ok(1, 5000, 3, 2048)
    assert ok(1, 5000, 5, 819) and not ok(1, 5000, 5, 820)                         # C * k1 <= 4096
    assert ok(1, 5000, 4096, 1) and not ok(1, 5000, 4097, 1)
    assert ok(2, 300, 1, 300) and not ok(2, 300, 1, 301)                           # k1 <= N
    assert not ok(1, 100, 2, 0) and not ok(0, 100, 2, 10) and not ok(1, 100, 0, 10)
    assert ok(1, (1 << 30) - 1, 2, 10) and not ok(1, 1 << 30, 2, 10)               # N < 2^30


def test_product_refuses_cpu_tensors_and_bad_shapes():
    from snuffy_amd import SnuffyHipError
    with pytest.raises(SnuffyHipError):
        ops.multiclass_select(torch.zeros(1, 8, 2), 2)


class Stub:
    """EncoderLayer.run with the selection fixed and SF.encoder_layer replaced by a recorder (no library call is made)."""

    def __init__(self, monkeypatch, layer, k):
        self.calls = []
        self.k = k

        def select(c, layer_index=0):
            b = c.shape[0]
            half = torch.arange(k // 2, dtype=torch.int64).repeat(b, 1)
            return half, half + k // 2

        def encoder_layer(x2, sel, lyr, need_attn, precision, packed=None, **kw):
            self.calls.append((tuple(x2.shape), tuple(sel.shape), None if packed is None else tuple(packed.sizes)))
            h = lyr.self_attn.h
            attn = torch.zeros(1, h, x2.shape[0], sel.shape[0] // (packed.bags if packed is not None else 1)) if need_attn else None
            return SF.Parts(x2), attn

        monkeypatch.setattr(layer, "select", select)
        monkeypatch.setattr(SF, "encoder_layer", encoder_layer)
        monkeypatch.setattr(smc, "_packed_bags", lambda b, n, dev: type("P", (), {"sizes": [n] * b, "bags": b, "dev": torch.arange(
            0, (b + 1) * n, n, dtype=torch.int64)})())


def make_layer(D, h, lam=12, r=0.5):
    return smc.EncoderLayer(D, smc.MultiHeadedAttention(h, D), smc.PositionwiseFeedForward(D, 4 * D, "relu"), 2, 0.0, lam, r).eval()


def test_run_routing(monkeypatch):
    B, N, K = 3, 300, 12
    c = torch.zeros(B, N, 2)
    loop = lambda d, b=B: [((N, d), (K,), None)] * b

    layer = make_layer(128, 2)
    stub = Stub(monkeypatch, layer, K)
    monkeypatch.setattr(smc, "PACK_BATCH", True)
    with torch.no_grad():
        parts, attn = layer.run(torch.zeros(B, N, 128), c)
    assert stub.calls == [((B * N, 128), (B * K,), (N,) * B)]                      # ONE packed call
    assert tuple(attn.shape) == (B, 2, N, K) and not isinstance(parts, list)
    assert tuple(smc._rows(parts, B).shape) == (B, N, 128)

    # B = 1, training (autograd on), dk = 32, the switch off: today's calls, one per row
    for what in ("b1", "grad", "dk32", "off"):
        stub.calls.clear()
        lyr, d, b = layer, 128, B
        if what == "dk32":
            lyr, d = make_layer(64, 2), 64
            Stub.__init__(stub, monkeypatch, lyr, K)
        if what == "b1":
            b = 1
        monkeypatch.setattr(smc, "PACK_BATCH", what != "off")
        with (torch.enable_grad() if what == "grad" else torch.no_grad()):
            parts, attn = lyr.run(torch.zeros(b, N, d), c[:b])
        assert stub.calls == loop(d, b), what
        assert isinstance(parts, list) and len(parts) == b and tuple(attn.shape) == (b, 2, N, K), what


def test_fused_select_switch_off_gives_the_old_calls(monkeypatch):
    """FUSED_SELECT = False (and any shape outside the kernel) never reaches ops.multiclass_select."""
    layer = make_layer(64, 2)
    seen = []
    monkeypatch.setattr(layer, "select_unfused", lambda c: seen.append("unfused") or ("t", "r"))
    monkeypatch.setattr(ops, "multiclass_select", lambda *a: (_ for _ in ()).throw(AssertionError("fused selector called")))
    monkeypatch.setattr(smc, "FUSED_SELECT", False)
    assert layer.select(torch.zeros(2, 60, 2)) == ("t", "r")
    monkeypatch.setattr(smc, "FUSED_SELECT", True)
    layer.big_lambda, layer.top_big_lambda_share = 8194, 1.0                        # C * k1 = 16388
    assert layer.select(torch.zeros(1, 9000, 2)) == ("t", "r")
    assert seen == ["unfused", "unfused"]
    assert not hasattr(smc, "build_milnet")


def test_new_kernels_keep_their_scratch():
    import scan_spills
    objdir = os.path.join(scan_spills.ROOT, "snuffy_amd", "build")
    if not os.path.isdir(objdir) or not os.path.exists(os.path.join(objdir, "topk.o")):
        pytest.skip("no build objects here (the library was built elsewhere)")
    try:
        ks = scan_spills.kernels(objdir)
    except RuntimeError as exc:
        pytest.skip(str(exc))
    names = scan_spills.demangle([k[1] for k in ks])
    sel, smp, radix64 = {}, {}, None
    for (obj, _, scratch, _, _), name in zip(ks, names):
        if "multiclass_select_kernel<" in name:
            sel[int(name.split("<", 1)[1].split(">")[0])] = scratch
        elif "sampler_keys_batched_kernel" in name or "sampler_exclude_batched_kernel" in name:
            smp[name.split("::")[-1].split("(")[0]] = scratch
        elif "topk_radix_kernel<64>" in name:
            radix64 = scratch
    assert sorted(sel) == [0, 8, 16, 32, 64] and radix64 is not None
    assert [sel[i] for i in (8, 16, 32, 0)] == [0, 0, 0, 0]
    assert sel[64] <= radix64, (sel[64], radix64)
    assert smp == {"sampler_keys_batched_kernel": 0, "sampler_exclude_batched_kernel": 0}
