"""The packed device sampler, the part that needs no GPU: the --sampler flag of train.py, the routing of packed.forward_packed_raw (with
the kernels stubbed) and the scratch bytes of the selector kernels in the built objects."""
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

from snuffy_amd import functional as SF
from snuffy_amd import ops, packed, snuffy, train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_train_flag_defaults_to_the_reference_sampler():
    p = train.get_args_parser()
    assert p.parse_args([]).sampler == "reference"
    assert p.parse_args(["--sampler", "device"]).sampler == "device"
    with pytest.raises(SystemExit):
        p.parse_args(["--sampler", "numpy"])


@pytest.mark.parametrize("flag", ["reference", "device"])
def test_trainer_passes_the_sampler_to_configure(monkeypatch, flag):
    seen = []
    real = snuffy.MILNet.configure

    def configure(self, *a, **kw):
        seen.append(kw)
        return real(self, *a, **kw)

    monkeypatch.setattr(snuffy.MILNet, "configure", configure)
    monkeypatch.setattr(train, "device", torch.device("cpu"))
    args = train.get_args_parser().parse_args(["--sampler", flag, "--feats_size", "32", "--num_heads", "2", "--big_lambda", "8",
                                               "--random_patch_share", "0.5"])
    fake = types.SimpleNamespace(args=args)
    net = train.Snuffy._get_milnet(fake)
    assert len(seen) == 1 and seen[0]["sampler"] == flag
    assert net.b_classifier.cfg.sampler == flag


def test_draw_packed_predicate_domain_edges():
    ok = ops.draw_packed_supported
    assert ok(1, 1, 1, 1) and ok(65536, 24, 2048, 4096)
    assert not ok(65537, 24, 40, 5) and not ok(0, 24, 40, 5)
    assert not ok(1000, 24, 2049, 5) and not ok(1000, 24, 0, 5) and not ok(1000, 0, 40, 5)
    assert not ok(1000, 24, 40, 0) and not ok(1000, 24, 40, 4097)


class Stub:
    """forward_packed_raw with every library call replaced: the critic, the segmented top-k, the layers and the head are recorders."""

    def __init__(self, monkeypatch, net, sizes, k1):
        self.draws, self.choices = [], 0
        b = len(sizes)
        monkeypatch.setattr(SF, "as_2d", lambda x: x)
        monkeypatch.setattr(SF, "critic_scores_with_hl", lambda x, w, bias, layer: torch.zeros(x.shape[0], 1))
        monkeypatch.setattr(ops, "topk_segmented", lambda c, pk, k: torch.arange(k, dtype=torch.int64).repeat(b, 1))
        monkeypatch.setattr(SF, "encoder_layer", lambda x2, sel, layer, need_attn, precision, packed=None, ragged=None: (x2, None))
        monkeypatch.setattr(SF, "materialize", lambda parts: parts)
        monkeypatch.setattr(SF, "head", lambda parts, norm, linear, packed=None: torch.zeros(b, 1))

        stub = self

        class Sampler:
            def draw_packed(self, pk, k1_, k2, top, layers):
                stub.draws.append((tuple(pk.sizes), k1_, k2, tuple(top.shape), layers))
                return (k1_ + torch.arange(k2, dtype=torch.int64)).repeat(layers, b, 1)

        monkeypatch.setattr(net.b_classifier.cfg, "device_sampler", lambda device: Sampler())
        choice = np.random.choice

        def counted(*a, **kw):
            stub.choices += 1
            return choice(*a, **kw)

        monkeypatch.setattr(np.random, "choice", counted)


def _packed_stub(sizes):
    host = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum(sizes, out=host[1:])
    return types.SimpleNamespace(sizes=list(sizes), bags=len(sizes), max_n=max(sizes), total=int(host[-1]), host=host,
                                 dev=torch.from_numpy(host), device=torch.device("cpu"), _plans={})


def test_forward_packed_raw_routing(monkeypatch):
    lam, r, depth, sizes = 8, 0.5, 3, [8, 30, 17]
    k1, k2 = math.ceil(lam * (1 - r)), int(lam * r)
    net = snuffy.build_milnet(32, 2, "relu", lam, r, depth).eval()
    stub = Stub(monkeypatch, net, sizes, k1)
    pk = _packed_stub(sizes)
    x = torch.zeros(pk.total, 32)
    monkeypatch.setattr(packed, "PACK_DEVICE_SAMPLER", True)

    net.configure(sampler="device")
    state = np.random.get_state()
    with torch.no_grad():
        packed.forward_packed_raw(net, x, pk)
    assert stub.draws == [(tuple(sizes), k1, k2, (3, k1), depth)] and stub.choices == 0      # ONE call for all layers and bags
    assert np.array_equal(state[1], np.random.get_state()[1]) and state[2] == np.random.get_state()[2]
    for li, layer in enumerate(net.b_classifier.encoder.layers):
        top, rnd = layer.last_selection_bags
        assert tuple(top.shape) == (3, k1) and tuple(rnd.shape) == (3, k2)

    # the reference sampler, and the device sampler with the switch off: numpy draws per bag and layer, never draw_packed
    for what in ("reference", "off"):
        stub.draws.clear()
        stub.choices = 0
        net.configure(sampler="reference" if what == "reference" else "device")
        monkeypatch.setattr(packed, "PACK_DEVICE_SAMPLER", what != "off")
        with torch.no_grad():
            packed.forward_packed_raw(net, x, pk)
        assert stub.draws == [] and stub.choices == depth * len(sizes), what

    # a uniform group with a bag shorter than Lambda is refused rather than read past its draws
    monkeypatch.setattr(packed, "PACK_DEVICE_SAMPLER", True)
    net.configure(sampler="device")
    with pytest.raises(SF.SnuffyHipError):
        packed.forward_packed_raw(net, torch.zeros(7 + 30, 32), _packed_stub([7, 30]))


def test_ragged_random_index_lists_the_valid_entries():
    k1, k2, sizes = 4, 4, [2, 4, 6, 8, 20]
    pk = _packed_stub(sizes)
    rag = types.SimpleNamespace(kbs=[min(k1 + k2, n) for n in sizes])
    pos, base = packed.ragged_random_index(pk, rag, k1, k2)
    want = [0, 1, 8, 9, 10, 11, 16, 17, 18, 19, 20, 21, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39]
    assert pos.tolist() == want
    assert base.tolist() == [0] * 2 + [2] * 4 + [6] * 6 + [12] * 8 + [20] * 8
    assert packed.ragged_random_index(pk, rag, k1, k2)[0] is pos                         # cached on the PackedBags


# scratch bytes per lane and VGPRs of the selector kernels before the packed sampler was added (tools/scan_spills.py)
BEFORE = {"topk_radix_kernel": {8: (0, 65), 16: (0, 73), 32: (0, 96), 64: (340, 128), 0: (0, 74)},
          "topk_radix_segmented_kernel": {8: (0, 65), 16: (0, 73), 32: (0, 96), 64: (336, 128), 0: (0, 56)}}


def test_selector_kernels_keep_their_scratch():
    import scan_spills
    objdir = os.path.join(scan_spills.ROOT, "snuffy_amd", "build")
    if not os.path.isdir(objdir) or not os.path.exists(os.path.join(objdir, "topk.o")):
        pytest.skip("no build objects here (the library was built elsewhere)")
    try:
        ks = scan_spills.kernels(objdir)
    except RuntimeError as exc:
        pytest.skip(str(exc))
    names = scan_spills.demangle([k[1] for k in ks])
    draw, old = {}, {k: {} for k in BEFORE}
    for (obj, _, scratch, _, vgpr), name in zip(ks, names):
        if "random_share_draw_kernel<" in name:
            draw[int(name.split("<", 1)[1].split(">")[0])] = scratch
        for k in BEFORE:
            if "::" + k + "<" in name:
                old[k][int(name.split("<", 1)[1].split(">")[0])] = (scratch, vgpr)
    assert draw == {8: 0, 16: 0, 32: 0}                      # no 64-key register form: longer bags take the key image
    assert old == BEFORE
