"""Packed (varlen) bf16 inference at head width 192 (the README's MAE recipe: D = 768, h = 4, Lambda = 500 as 250 + 250).
Kernel level: the varlen launches of the width (1, 2, 4 key blocks; key chunks of 2 / 4 blocks) against the single-bag entry point
(same P and lse bit for bit, O up to the fp32 order of the partial sums), independent of the batch composition bit for bit, against
fp64, and bit-identical on a repeat.  Model level: MILNet.forward_bags with packed.PACK_DK192 on against the per-bag forwards and the
CPU oracle, with the device sampler (one group, a mix with a short bag, graph replay), and the routing of before with the switch off
and at precision="fp32"."""
import numpy as np
import pytest
import torch

from oracle import snuffy_oracle as orc
from tests.attn_widths import (OFFSET, VARLEN_192 as ROW, _bags, _close, _fp64_reference, _loop, _offset, _packed, _place_sampler,
                               _sizes, device_sampler_on, op, single_bag, y_bound)  # noqa: F401  (fixtures)
from tests.helpers import build_amd_milnet

pytestmark = pytest.mark.gpu
DEV = "cuda"

D_K, H_K = ROW.D_K, ROW.H_K                       # kernel level: the smallest model width with dk = 192
KEYS = ROW.KEYS


@pytest.mark.parametrize("k", KEYS)
@pytest.mark.parametrize("need_attn", [False, True])
def test_attention_varlen_dk192_vs_per_bag_and_composition_independent(k, need_attn):
    from snuffy_amd import ops
    d, h = D_K, H_K
    sizes = _sizes(k)
    pk = _packed(sizes)
    g = torch.Generator().manual_seed(1)
    qv = torch.randn(pk.total, 2 * d, generator=g).to(DEV).to(torch.bfloat16)
    kp = (torch.randn(pk.bags * k, d, generator=g) * 0.5).to(DEV).to(torch.bfloat16)
    assert op(ROW, "varlen_supported")(k) and not ops.varlen_attn_chunks_supported(ROW.kind, k, d // h)
    varlen = op(ROW, "varlen")
    q, v = qv[:, :d], qv[:, d:]
    out, attn, lse = varlen(q, v, kp, pk, k, h, need_attn=need_attn, need_lse=need_attn)
    assert out.shape == (pk.bags * k, d)
    for b, n in enumerate(sizes):
        lo = int(pk.host[b])
        qb, kb = qv[lo:lo + n], kp[b * k:(b + 1) * k]
        o1, a1, l1 = single_bag(ROW, qb[:, :d], qb[:, d:], kb, h, need_attn=need_attn, need_lse=need_attn)
        err, ref = (out[b * k:(b + 1) * k] - o1).abs().max().item(), o1.abs().max().item()
        print("dk=192 k=%d bag %d n=%d: |out - single| / max|out| = %.3g" % (k, b, n, err / ref))
        # the single-bag entry point spreads a small bag over more workgroups: same P, O up to the fp32 order of the partial sums
        assert err <= 2e-6 * ref, (b, n)
        if need_attn:
            assert torch.equal(attn[:, lo:lo + n], a1), (b, n)
            assert torch.equal(lse[:, lo:lo + n], l1), (b, n)
        # a bag's result does not depend on what it is packed with: alone in a varlen launch, bit for bit
        o2, a2, l2 = varlen(qb[:, :d], qb[:, d:], kb, _packed([n]), k, h, need_attn=need_attn, need_lse=need_attn)
        assert torch.equal(out[b * k:(b + 1) * k], o2), (b, n)
        if need_attn:
            assert torch.equal(attn[:, lo:lo + n], a2) and torch.equal(lse[:, lo:lo + n], l2), (b, n)
    # against fp64 on one bag (the kernels agree with each other; this pins them to the definition)
    b = 1
    lo, n = int(pk.host[b]), sizes[b]
    ref = _fp64_reference((ROW.id, k), qv[lo:lo + n, :d], qv[lo:lo + n, d:], kp[b * k:(b + 1) * k], h)
    err = (out[b * k:(b + 1) * k].double() - ref).abs().max().item() / ref.abs().max().item()
    print("dk=192 k=%d: relative error against fp64 %.3g" % (k, err))
    assert err < ROW.O_FP64[k > 256], err
    # a repeat call is bit-identical
    out_r, attn_r, lse_r = varlen(q, v, kp, pk, k, h, need_attn=need_attn, need_lse=need_attn)
    assert torch.equal(out, out_r)
    if need_attn:
        assert torch.equal(attn, attn_r) and torch.equal(lse, lse_r)


# ---- model level ----------------------------------------------------------------------------------------------------------------------
D, H, LAM, R, ACT = ROW.D, ROW.H, ROW.LAM, ROW.R, ROW.ACT
SIZES = ROW.SIZES


def _net(precision="bf16", sampler=None, return_attention=True, seed=0):
    torch.manual_seed(seed)
    net = build_amd_milnet(D, H, ACT, LAM, R, 1).to(DEV).eval()
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() > 1:
                torch.nn.init.xavier_uniform_(p)
    if sampler is None:
        net.configure(precision=precision, return_attention=return_attention)
    else:
        net.configure(precision=precision, return_attention=return_attention, sampler=sampler)
    return net


@pytest.fixture
def dk192_on(monkeypatch):
    from snuffy_amd import packed
    monkeypatch.setattr(packed, ROW.pack_switch, True)              # the switch under test, whatever its shipped default


def _count_varlen_calls(monkeypatch):
    from snuffy_amd import ops
    calls, real = [], getattr(ops, ROW.varlen)

    def spy(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(ops, ROW.varlen, spy)
    return calls


@pytest.mark.parametrize("single_bag_mfma", [True, None])
def test_forward_bags_of_the_mae_recipe_matches_per_bag_forwards(dk192_on, monkeypatch, single_bag_mfma):
    """single_bag_mfma True: the loop runs the bf16 MFMA kernel of the width (functional.MFMA_ATTN_DK192 forced on); None: as shipped
    (off: the loop runs the exact kernel on bf16-rounded Q | V) -- the bf16 class holds either way."""
    from snuffy_amd import functional as SF
    if single_bag_mfma:
        monkeypatch.setattr(SF, ROW.single_switch, True)
    calls = _count_varlen_calls(monkeypatch)
    net = _net()
    bags = _bags(SIZES, D)
    with torch.no_grad():
        np.random.seed(11)
        ref, sel_ref = _loop(net, bags)
        assert not calls
        np.random.seed(11)
        assert net._packable(bags)
        got = net.forward_bags(bags)
        assert len(calls) == 1
        after_packed = np.random.rand()
        np.random.seed(11)
        [net(x) for x in bags]
        assert np.random.rand() == after_packed          # the numpy stream is left where the per-bag loop leaves it
    top, rnd = net.b_classifier.encoder.layers[0].last_selection_bags
    for b in range(len(bags)):                           # selections, random share included: bit-exact
        assert torch.equal(top[b], sel_ref[b][0][0]) and torch.equal(rnd[b], sel_ref[b][0][1])
        _close(ROW, ref[b], got[b], SIZES[b])


def test_forward_bags_of_the_mae_recipe_vs_oracle(dk192_on):
    sizes = ROW.ORACLE_SIZES
    net = _net()
    bags = _bags(sizes, D, seed=9)
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        np.random.seed(3)
        assert net._packable(bags)
        got = net.forward_bags(bags)
    top, rnd = net.b_classifier.encoder.layers[0].last_selection_bags
    for b, x in enumerate(bags):
        sel = torch.cat((top[b], rnd[b])).cpu()
        classes, logits, attn, _ = orc.milnet_forward(x[0].cpu(), sd, H, ACT, LAM, R, 1, forced_sel=[sel])
        own_top, _ = orc.select_indices(classes[:, 0], LAM, R, np.random.RandomState(0))
        assert np.array_equal(own_top.numpy(), top[b].cpu().numpy())                   # bit-exact top indices per bag
        dy, da = (got[b][1][0].cpu() - logits).abs().max().item(), (got[b][2][0].cpu() - attn).abs().max().item()
        print("bag %d against the oracle: |dlogit| %.3g  |dA| %.3g" % (b, dy, da))
        assert dy <= y_bound(ROW, logits)
        assert da <= ROW.A_TOL


def test_device_sampler_one_group_equals_the_loop(dk192_on, device_sampler_on):
    net = _net(sampler="device")
    bags = _bags(SIZES, D)
    with torch.no_grad():
        _place_sampler(net, OFFSET)
        ref, sel_ref = _loop(net, bags)
        _place_sampler(net, OFFSET)
        assert net._packable(bags)
        got = net.forward_bags(bags)
        assert _offset(net) == OFFSET + len(bags)
    top, rnd = net.b_classifier.encoder.layers[0].last_selection_bags
    for b in range(len(bags)):
        assert torch.equal(top[b], sel_ref[b][0][0]) and torch.equal(rnd[b], sel_ref[b][0][1]), b
        _close(ROW, ref[b], got[b], SIZES[b])


def test_device_sampler_mix_with_a_short_bag(dk192_on, device_sampler_on):
    """A 150-row bag (shorter than Lambda: it selects all of its rows, 150 keys) next to the uniform group: pack_groups leaves it to the
    per-bag loop (a ragged group needs two bags), which runs after the group and draws from the next offset."""
    sizes = ROW.MIX_SIZES
    net = _net(sampler="device")
    bags = _bags(sizes, D, seed=17)
    with torch.no_grad():
        groups = net._pack_groups(bags)
        assert groups == [([0, 2, 3], False)]
        offsets = {0: OFFSET + 1, 2: OFFSET + 2, 3: OFFSET + 3, 1: OFFSET + 4}
        _place_sampler(net, OFFSET)
        got = net.forward_bags(bags)
        assert _offset(net) == OFFSET + len(bags)
        for i, x in enumerate(bags):
            _place_sampler(net, offsets[i] - 1)                 # the one-bag forward advances before it draws
            c0, y0, a0 = net(x)
            c1, y1, a1 = got[i]
            assert a1.shape == a0.shape == (1, H, sizes[i], min(LAM, sizes[i]))
            assert torch.equal(c0, c1)
            assert (y0 - y1).abs().max().item() <= y_bound(ROW, y0), i
            assert (a0 - a1).abs().max().item() <= ROW.A_TOL, i
        # two short bags form a ragged group behind the uniform one (150 keys: inside the ragged kernel at this width)
        bags2 = bags + _bags([160], D, seed=19)
        assert net._pack_groups(bags2) == [([0, 2, 3], False), ([1, 4], True)]


def test_device_sampler_graph_replay_draws_fresh_rows(dk192_on, device_sampler_on):
    sizes = ROW.GRAPH_SIZES
    B = len(sizes)
    net = _net(sampler="device", return_attention=False)
    net.configure(sampler="device", graph_max_patches=1 << 20, return_attention=False)
    bags = _bags(sizes, D, seed=21)
    _place_sampler(net, OFFSET)
    # call 1 is eager (the composition is remembered), call 2 warms up twice, captures and replays, call 3 replays only
    starts = [OFFSET, OFFSET + 3 * B, OFFSET + 4 * B]
    sels, outs = [], []
    with torch.no_grad():
        for call in range(3):
            got = net.forward_bags(bags)
            assert any(k and k[0] == "bags" for k in net._graphs) == (call >= 1)
            assert _offset(net) == starts[call] + B, call
            sels.append(net.b_classifier.encoder.layers[0].last_selection_bags[1].cpu().numpy().copy())
            outs.append([y.clone() for _, y, _ in got])
        assert sum(1 for k in net._graphs if k and k[0] == "bags") == 1
        assert not np.array_equal(sels[1], sels[2]) and not np.array_equal(sels[0], sels[1])
        net.configure(graph_max_patches=0)
        _place_sampler(net, starts[2])
        eager = net.forward_bags(bags)                        # the eager issue from the last replay's record: bit for bit
    assert not net._graphs
    assert np.array_equal(net.b_classifier.encoder.layers[0].last_selection_bags[1].cpu().numpy(), sels[2])
    for b in range(B):
        assert torch.equal(eager[b][1], outs[2][b])


def test_switch_off_keeps_the_per_bag_loop(monkeypatch):
    from snuffy_amd import packed
    monkeypatch.setattr(packed, ROW.pack_switch, False)
    calls = _count_varlen_calls(monkeypatch)
    net = _net()
    bags = _bags(ROW.OFF_SIZES, D, seed=13)
    with torch.no_grad():
        assert not net._packable(bags) and net._pack_groups(bags) is None
        np.random.seed(11)
        got = net.forward_bags(bags)
        np.random.seed(11)
        ref = [net(x) for x in bags]
    assert not calls
    for (c0, y0, a0), (c1, y1, a1) in zip(ref, got):
        assert torch.equal(c0, c1) and torch.equal(y0, y1) and torch.equal(a0, a1)


@pytest.mark.parametrize("on", [True, False])
def test_fp32_stays_per_bag_whatever_the_switch(monkeypatch, on):
    from snuffy_amd import packed
    monkeypatch.setattr(packed, ROW.pack_switch, on)
    calls = _count_varlen_calls(monkeypatch)
    net = _net(precision="fp32")
    bags = _bags([600, 1100], D, seed=13)
    with torch.no_grad():
        assert net._pack_groups(bags) is None
        np.random.seed(11)
        got = net.forward_bags(bags)
        np.random.seed(11)
        ref = [net(x) for x in bags]
    assert not calls
    for (c0, y0, a0), (c1, y1, a1) in zip(ref, got):
        assert torch.equal(c0, c1) and torch.equal(y0, y1) and torch.equal(a0, a1)
