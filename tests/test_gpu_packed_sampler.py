"""The random patch share of the packed (varlen) inference path drawn on the device: the one-launch draw kernel against its host twin
(oracle/philox_ref.py) and against the one-bag sampler, MILNet.forward_bags under configure(sampler="device") against the per-bag loop
and the CPU oracle, graph replay with fresh draws, several groups (uniform + ragged), and the switch."""
import numpy as np
import pytest
import torch

from oracle import philox_ref
from oracle import snuffy_oracle as orc
from tests.attn_widths import OFFSET, SEED, _bags, _loop, _offset, _place_sampler
from tests.attn_widths import outputs_close as _close
from tests.helpers import build_amd_milnet

pytestmark = pytest.mark.gpu
DEV = "cuda"
KERNEL_SIZES = [1, 23, 24, 25, 63, 64, 65, 1023, 1025, 4097, 8192, 8193, 16385, 32769, 65536]


def _k2b(n, k1, k2):
    return min(k2, max(0, n - k1))


def _check_draws(sizes, k1, k2, layers, one_bag_sampler=True):
    from snuffy_amd import ops
    pk = ops.PackedBags(sizes, DEV)
    g = torch.Generator().manual_seed(3)
    scores = torch.randn(pk.total, generator=g).to(DEV)
    top = ops.topk_segmented(scores, pk, k1)
    smp = ops.DeviceSampler(DEV, SEED, OFFSET)
    assert ops.draw_packed_supported(pk.max_n, k1, k2, layers)
    rnd = smp.draw_packed(pk, k1, k2, top, layers)
    assert tuple(rnd.shape) == (layers, len(sizes), k2) and rnd.dtype == torch.int64
    assert smp.state.cpu().tolist() == [SEED, OFFSET + len(sizes)]              # advanced by B on the device
    top_h, rnd_h = top.cpu().numpy(), rnd.cpu().numpy()
    for b, n in enumerate(sizes):
        kb, tb = _k2b(n, k1, k2), top_h[b, :min(k1, n)]
        one = ops.DeviceSampler(DEV, SEED, OFFSET + 1 + b) if one_bag_sampler and kb else None
        for l in range(layers):
            want = philox_ref.random_share_draw(n, kb, SEED, OFFSET + 1 + b, l, tb)
            assert np.array_equal(rnd_h[l, b, :kb], want), (b, n, l)
            assert len(set(want.tolist())) == kb and not set(want.tolist()) & set(tb.tolist())
            if one is not None:
                assert torch.equal(one.draw(n, kb, top[b, :min(k1, n)].contiguous(), layer=l), rnd[l, b, :kb]), (b, n, l)


@pytest.mark.parametrize("max_n", [65536, 32768, 16384, 8192])
def test_draw_kernel_matches_the_host_twin(max_n):
    """k1 = 24, k2 = 40, 5 layers over bag sizes with no draw at all (n <= k1), a short draw (k2_b < k2), n = k1 + k2 exactly, rows that
    are no multiple of 4, and the thread / register-class boundaries.  The full list runs as one call (its longest bag puts the call on
    the key-image form); the lists cut at 8 k / 16 k / 32 k rows run the three register forms."""
    _check_draws([n for n in KERNEL_SIZES if n <= max_n], 24, 40, 5)


def test_draw_kernel_has_no_bag_count_limit():
    _check_draws([300] * 70, 24, 40, 5)                                        # above draw_batch's 64 rows: bags differ by offset


def test_draw_packed_refuses_what_is_outside_the_kernel():
    from snuffy_amd import SnuffyHipError, ops
    pk = ops.PackedBags([100, 70000], DEV)
    smp = ops.DeviceSampler(DEV, SEED, OFFSET)
    top = torch.zeros(2, 8, dtype=torch.int64, device=DEV)
    assert not ops.draw_packed_supported(pk.max_n, 8, 8, 1) and not ops.draw_packed_supported(100, 8, 2049, 1)
    with pytest.raises(SnuffyHipError):
        smp.draw_packed(pk, 8, 8, top, 1)
    assert smp.state.cpu().tolist() == [SEED, OFFSET]


# ---- model level ----------------------------------------------------------------------------------------------------
def _net(d, h, lam, r, depth, precision, seed=0, return_attention=True):
    torch.manual_seed(seed)
    net = build_amd_milnet(d, h, "relu", lam, r, depth).to(DEV).eval()
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() > 1:
                torch.nn.init.xavier_uniform_(p)
    net.configure(precision=precision, return_attention=return_attention, sampler="device")
    return net


@pytest.fixture(autouse=True)
def _switch_on(monkeypatch):
    """The model-level tests cover the device-sampler route whatever value the switch ships with."""
    from snuffy_amd import packed
    monkeypatch.setattr(packed, "PACK_DEVICE_SAMPLER", True)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("lam,r,depth", [(64, 0.25, 2), (200, 0.5, 1)])
def test_forward_bags_draws_what_the_per_bag_loop_draws(precision, lam, r, depth):
    """One uniform group over all bags in order: bag b's packed draw is the b-th per-bag forward's, bit for bit, numpy's stream is not
    touched and the record ends B further on."""
    d, sizes = 384, [lam, 1000, 333, 4100, 2048]
    net = _net(d, 6, lam, r, depth, precision)
    bags = _bags(sizes, d)
    with torch.no_grad():
        _place_sampler(net, OFFSET)
        ref, sel_ref = _loop(net, bags)
        assert _offset(net) == OFFSET + len(bags)
        _place_sampler(net, OFFSET)
        assert net._packable(bags)
        np.random.seed(11)
        before = np.random.get_state()
        got = net.forward_bags(bags)
        after = np.random.get_state()
        assert _offset(net) == OFFSET + len(bags)
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    for li, layer in enumerate(net.b_classifier.encoder.layers):
        top, rnd = layer.last_selection_bags
        for b in range(len(bags)):
            assert torch.equal(top[b], sel_ref[b][li][0]) and torch.equal(rnd[b], sel_ref[b][li][1]), (li, b)
    for b in range(len(bags)):
        _close(ref[b], got[b], precision)


def test_forward_bags_device_draws_vs_oracle():
    d, h, lam, r, depth = 384, 6, 64, 0.25, 2
    sizes = [lam, 1000, 333, 4100, 2048]
    net = _net(d, h, lam, r, depth, "fp32")
    bags = _bags(sizes, d)
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        _place_sampler(net, OFFSET)
        got = net.forward_bags(bags)
    b = 2
    sels = [torch.cat((l.last_selection_bags[0][b], l.last_selection_bags[1][b])).cpu() for l in net.b_classifier.encoder.layers]
    classes, logits, attn, _ = orc.milnet_forward(bags[b][0].cpu(), sd, h, "relu", lam, r, depth, forced_sel=sels)
    own_top, _ = orc.select_indices(classes[:, 0], lam, r, np.random.RandomState(0))
    assert np.array_equal(own_top.numpy(), net.b_classifier.encoder.layers[0].last_selection_bags[0][b].cpu().numpy())
    assert (got[b][1][0].cpu() - logits).abs().max().item() <= 1e-3 * max(1.0, logits.abs().max().item())
    assert (got[b][2][0].cpu() - attn).abs().max().item() <= 1e-3


def _twin_matches(layers_sel, sizes, k1, k2, offsets):
    """layers_sel: per layer (top [B, k1], rnd [B, k2]) as host arrays; bag b drew from offsets[b]."""
    for l, (top, rnd) in enumerate(layers_sel):
        for b, n in enumerate(sizes):
            kb = _k2b(n, k1, k2)
            want = philox_ref.random_share_draw(n, kb, SEED, offsets[b], l, top[b, :min(k1, n)])
            assert np.array_equal(rnd[b, :kb], want), (l, b)


def test_graph_replay_draws_fresh_rows():
    d, lam, r = 384, 200, 0.5
    sizes = [600, 1500, 900, 1200]
    B = len(sizes)
    net = _net(d, 6, lam, r, 1, "bf16", return_attention=False)
    net.configure(sampler="device", graph_max_patches=1 << 20, return_attention=False)
    bags = _bags(sizes, d, seed=21)
    _place_sampler(net, OFFSET)
    # call 1 is eager (the composition is remembered), call 2 warms up twice, captures and replays, calls 3 - 5 replay only
    starts = [OFFSET, OFFSET + 3 * B, OFFSET + 4 * B, OFFSET + 5 * B, OFFSET + 6 * B]
    sels, outs = [], []
    with torch.no_grad():
        for call in range(5):
            got = net.forward_bags(bags)
            assert any(k and k[0] == "bags" for k in net._graphs) == (call >= 1)
            assert _offset(net) == starts[call] + B, call
            sels.append([tuple(t.cpu().numpy().copy() for t in l.last_selection_bags) for l in net.b_classifier.encoder.layers])
            outs.append([y.clone() for _, y, _ in got])
    assert sum(1 for k in net._graphs if k and k[0] == "bags") == 1
    for call in range(5):
        _twin_matches(sels[call], sizes, 100, 100, [starts[call] + 1 + b for b in range(B)])
    for i, j in ((2, 3), (2, 4), (3, 4)):
        assert not np.array_equal(sels[i][0][1], sels[j][0][1])
    with torch.no_grad():
        net.configure(graph_max_patches=0)
        _place_sampler(net, starts[4])
        eager = net.forward_bags(bags)
    assert not net._graphs
    for b in range(B):
        assert torch.equal(eager[b][1], outs[4][b])


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_several_groups_follow_the_documented_offset_order(precision):
    from snuffy_amd import SnuffyHipError, ops
    d, h, lam, r, depth = 128, 2, 40, 0.5, 2
    k1 = k2 = 20
    sizes = [10, 20, 39, 40, 41, 300, 1000]
    net = _net(d, h, lam, r, depth, precision)
    bags = _bags(sizes, d, seed=17)
    with torch.no_grad():
        groups = net._pack_groups(bags)
        assert groups == [([3, 4, 5, 6], False), ([0, 1, 2], True)]
        # the uniform group runs first and takes one offset per bag, the ragged group follows
        offsets = {3: OFFSET + 1, 4: OFFSET + 2, 5: OFFSET + 3, 6: OFFSET + 4, 0: OFFSET + 5, 1: OFFSET + 6, 2: OFFSET + 7}
        _place_sampler(net, OFFSET)
        seen = {}
        from snuffy_amd import packed as pkd
        raw = pkd.forward_packed_raw

        def spy(net_, x_cat, packed, ragged=False):
            res = raw(net_, x_cat, packed, ragged)
            seen[bool(ragged)] = [tuple(t.cpu().numpy().copy() for t in l.last_selection_bags) for l in net_.b_classifier.encoder.layers]
            return res

        pkd.forward_packed_raw = spy
        try:
            got = net.forward_bags(bags)
        finally:
            pkd.forward_packed_raw = raw
        assert _offset(net) == OFFSET + len(bags)
        for (idx, ragged) in groups:
            _twin_matches(seen[ragged], [sizes[i] for i in idx], k1, k2, [offsets[i] for i in idx])
        for i, x in enumerate(bags):
            _place_sampler(net, offsets[i] - 1)                 # the one-bag forward advances before it draws
            _close(net(x), got[i], precision)
        # the reference sampler's draws stay out of ragged groups
        net.configure(sampler="reference")
        assert net._pack_groups(bags) is None
        idx = [0, 1, 2]
        pk = ops.PackedBags([sizes[i] for i in idx], DEV)
        with pytest.raises(SnuffyHipError):
            net.forward_packed(torch.cat([bags[i][0] for i in idx]), pk, ragged=True)


def test_switch_off_keeps_the_host_draws(monkeypatch):
    from snuffy_amd import packed
    d, lam, r = 384, 64, 0.25
    sizes = [64, 500, 333]
    net = _net(d, 6, lam, r, 2, "bf16")
    bags = _bags(sizes, d)
    monkeypatch.setattr(packed, "PACK_DEVICE_SAMPLER", False)
    with torch.no_grad():
        _place_sampler(net, OFFSET)
        np.random.seed(11)
        net.forward_bags(bags)
        after_device = np.random.rand()
        assert _offset(net) == OFFSET                           # the device record is not used
        sel_dev = [l.last_selection_bags[1].clone() for l in net.b_classifier.encoder.layers]
        net.configure(sampler="reference")
        np.random.seed(11)
        net.forward_bags(bags)
        assert np.random.rand() == after_device                 # numpy's stream consumed exactly as under the reference sampler
        np.random.seed(11)
        assert np.random.rand() != after_device
    for li, l in enumerate(net.b_classifier.encoder.layers):
        assert torch.equal(l.last_selection_bags[1], sel_dev[li])
