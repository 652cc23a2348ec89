"""The bf16 MFMA sparse attention at head width 256 (the README's SimCLR ResNet-18 recipe: D = 512, h = 2, Lambda = 900 as 200 + 700,
gelu, one encoder layer, precision="bf16"), single bag and packed.
Kernel level: the single-bag entry point with the checks and bounds of tests/test_gpu_attn_dk192.py::test_forward, unchanged; the varlen
launches with those of test_attention_varlen_dk192_vs_per_bag_and_composition_independent.
Model level: the single bag behind functional.MFMA_ATTN_DK256 (call lists by spies, selections, the CPU oracle), a deep stack (which runs
the fp32-class kernels whatever precision says), MILNet.forward_bags behind packed.PACK_DK256 against the per-bag forwards and the CPU
oracle, the device sampler (one group, a mix with a short bag, graph replay), and the routing that ships."""
import numpy as np
import pytest
import torch

from oracle import snuffy_oracle as orc
from tests.attn_widths import (OFFSET, MFMA_256 as ROW, _bags, _close, _fp64_reference, _loop, _offset, _packed, _place_sampler,
                               _sizes, _spy, device_sampler_on, op, pack_on, y_bound)  # noqa: F401  (fixtures)
from tests.helpers import ReplayRNG, _ops, _qv, attn_ref, bf16r, build_amd_milnet, rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture
def row():
    return ROW
DEV = "cuda"
BF = torch.bfloat16
DK = ROW.dk


# ---- single bag, kernel level -----------------------------------------------------------------------------------------------------------
SHAPES = ROW.SHAPES


@pytest.mark.parametrize("n,k,h", SHAPES)
def test_forward(n, k, h):
    """The checks of test_gpu_attn_dk192.py::test_forward at dk = 256 (bf16 Q | V only).  Without the kernel the first call fails: the
    entry point does not exist."""
    ops = _ops()
    assert op(ROW, "single_supported")(k, n, 2 * h * DK) and not ops.mfma_attn_supported(k, DK, n, 2 * h * DK)
    g = torch.Generator().manual_seed(n * 3 + k)
    d = h * DK
    q, kp, v = torch.randn(n, d, generator=g), torch.randn(k, d, generator=g), torch.randn(n, d, generator=g)
    qd, vd = _qv(q, v, "bf16")                                               # row-strided halves of one [n, 2d] buffer
    fwd = op(ROW, "single")
    o, attn, lse = fwd(qd, vd, kp.to(DEV), h, need_attn=True, need_lse=True)
    # (a) against the exact oracle: bf16-class tolerance
    o_ref, p_ref = attn_ref(q, kp, v, h)
    e_pa, e_oa = (attn.cpu().double() - p_ref).abs().max().item(), rel_err(o.cpu(), o_ref)
    # (b) against the oracle fed with the same bf16-rounded operands: tight (catches any layout slip)
    o_r, p_r = attn_ref(bf16r(q), bf16r(kp), bf16r(v), h)
    e_pb, e_ob = (attn.cpu().double() - p_r).abs().max().item(), rel_err(o.cpu(), o_r)
    e_s = (attn.sum(-1) - 1).abs().max().item()
    e_c = rel_err(o.cpu().view(k, h, DK).sum(0), bf16r(v).view(n, h, DK).sum(0))
    s_r = (bf16r(q).double().view(n, h, DK).transpose(0, 1) @ bf16r(kp).double().view(k, h, DK).transpose(0, 1).transpose(1, 2)) / DK ** 0.5
    e_l = (lse.cpu().double() - torch.logsumexp(s_r, -1)).abs().max().item()
    print("dk=256 n=%d k=%d h=%d: exact |dP| %.3g O %.3g; rounded operands |dP| %.3g (max P %.3g) O %.3g; |rowsum - 1| %.3g  colsum %.3g"
          "  |dlse| %.3g" % (n, k, h, e_pa, e_oa, e_pb, float(p_r.max()), e_ob, e_s, e_c, e_l))
    assert e_pa < 1e-2
    assert e_oa < 1e-2
    assert e_pb < 2e-5 + 2e-3 * float(p_r.max())
    assert e_ob < 3e-3
    # rows of P sum to one; sum over keys of O equals the column sums of V
    assert e_s < 1e-4
    assert e_c < 5e-3
    assert e_l < 1e-3
    # run-to-run determinism, contiguous operands
    o2, attn2, _ = fwd(q.to(DEV).to(BF), v.to(DEV).to(BF), kp.to(DEV), h, need_attn=True)
    assert torch.equal(o2, o) and torch.equal(attn2, attn)
    # without materialising A (need_attn=False, with and without lse) the output is the same
    o3, a3, l3 = fwd(qd, vd, kp.to(DEV), h)
    assert a3 is None and l3 is None and torch.equal(o3, o)
    o5, a5, l5 = fwd(qd, vd, kp.to(DEV), h, need_attn=False, need_lse=True)
    assert a5 is None and torch.equal(l5, lse) and torch.equal(o5, o)
    # a bf16 Kp is read as it is: same bits as the library's own round-to-nearest-even of the f32 Kp
    o4, a4, _ = fwd(qd, vd, kp.to(DEV).to(BF), h, need_attn=True)
    assert torch.equal(o4, o) and torch.equal(a4, attn)


def test_refusals_and_copied_views():
    from snuffy_amd import SnuffyHipError
    ops = _ops()
    fwd = op(ROW, "single")
    z = lambda *s: torch.zeros(*s, device=DEV, dtype=BF)                        # noqa: E731
    with pytest.raises(TypeError):
        fwd(z(64, 512).float(), z(64, 512).float(), z(8, 512), 2)               # f32 q / v
    with pytest.raises(SnuffyHipError):
        fwd(z(64, 512), z(64, 512), z(1025, 512), 2)                            # k = 1025
    with pytest.raises(SnuffyHipError):
        fwd(z(64, 256), z(64, 256), z(8, 256), 2)                               # d = 128 h
    with pytest.raises(SnuffyHipError):
        ops.sparse_attn_fwd_mfma(z(64, 512), z(64, 512), z(8, 512), 64, 2)      # the older entry point keeps refusing the width
    # a view _rows16 cannot take in place (rows start 2 bytes off a 16-byte boundary) is copied and answers as the contiguous operand
    n, k, h = 300, 50, 2
    g = torch.Generator().manual_seed(5)
    q, kp, v = (torch.randn(s, h * DK, generator=g) for s in (n, k, n))
    wide = torch.zeros(n, 2 * h * DK + 8, dtype=BF, device=DEV)
    wide[:, 1:1 + h * DK] = q.to(DEV).to(BF)
    wide[:, 1 + h * DK:1 + 2 * h * DK] = v.to(DEV).to(BF)
    qv_, vv_ = wide[:, 1:1 + h * DK], wide[:, 1 + h * DK:1 + 2 * h * DK]
    assert qv_.data_ptr() % 16 and not qv_.is_contiguous()
    o, a, _ = fwd(qv_, vv_, kp.to(DEV), h, need_attn=True)
    o0, a0, _ = fwd(q.to(DEV).to(BF), v.to(DEV).to(BF), kp.to(DEV), h, need_attn=True)
    assert torch.equal(o, o0) and torch.equal(a, a0)


# ---- varlen -----------------------------------------------------------------------------------------------------------------------------
KEYS = ROW.KEYS
D_K, H_K = ROW.D_K, ROW.H_K


@pytest.mark.parametrize("k", KEYS)
@pytest.mark.parametrize("need_attn", [False, True])
def test_attention_varlen_dk256_vs_per_bag_and_composition_independent(k, need_attn):
    ops = _ops()
    d, h = D_K, H_K
    sizes = _sizes(k)
    pk = _packed(sizes)
    g = torch.Generator().manual_seed(1)
    qv = torch.randn(pk.total, 2 * d, generator=g).to(DEV).to(BF)
    kp = (torch.randn(pk.bags * k, d, generator=g) * 0.5).to(DEV).to(BF)
    assert op(ROW, "varlen_supported")(k) and not ops.varlen_attn_chunks_supported(ROW.kind, k, d // h)
    varlen = op(ROW, "varlen")
    q, v = qv[:, :d], qv[:, d:]
    out, attn, lse = varlen(q, v, kp, pk, k, h, need_attn=need_attn, need_lse=need_attn)
    assert out.shape == (pk.bags * k, d)
    for b, n in enumerate(sizes):
        lo = int(pk.host[b])
        qb, kb = qv[lo:lo + n], kp[b * k:(b + 1) * k]
        o1, a1, l1 = op(ROW, "single")(qb[:, :d], qb[:, d:], kb, h, need_attn=need_attn, need_lse=need_attn)
        err, ref = (out[b * k:(b + 1) * k] - o1).abs().max().item(), o1.abs().max().item()
        print("dk=256 k=%d bag %d n=%d: |out - single| / max|out| = %.3g" % (k, b, n, err / ref))
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
    ref = _fp64_reference((ROW.id, k), qv[lo:lo + n, :d], qv[lo:lo + n, d:], kp[b * k:(b + 1) * k], h, oracle=True)
    err = (out[b * k:(b + 1) * k].double().cpu() - ref).abs().max().item() / ref.abs().max().item()
    print("dk=256 k=%d: relative error against fp64 %.3g" % (k, err))
    assert err < ROW.O_FP64[k > 256], err
    # a repeat call is bit-identical
    out_r, attn_r, lse_r = varlen(q, v, kp, pk, k, h, need_attn=need_attn, need_lse=need_attn)
    assert torch.equal(out, out_r)
    if need_attn:
        assert torch.equal(attn, attn_r) and torch.equal(lse, lse_r)


# ---- model level ------------------------------------------------------------------------------------------------------------------------
D, H, LAM, R, ACT = ROW.D, ROW.H, ROW.LAM, ROW.R, ROW.ACT
K_TOP = ROW.K_TOP                                 # 200 = ceil(900 (1 - 7/9)); the random share draws the other 700
SIZES = ROW.SIZES


def _net(sampler=None, return_attention=True, seed=0, depth=1, precision="bf16", lam=LAM, r=R):
    torch.manual_seed(seed)
    net = build_amd_milnet(D, H, ACT, lam, r, depth).to(DEV).eval()
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() > 1:
                torch.nn.init.xavier_uniform_(p)
    if sampler is None:
        net.configure(precision=precision, return_attention=return_attention)
    else:
        net.configure(precision=precision, return_attention=return_attention, sampler=sampler)
    return net


@pytest.mark.parametrize("lam,r", [(LAM, R),          # the recipe: eight key chunks
                                   (100, 0.0)])      # one chunk, no random share
def test_single_bag_routing_and_oracle(monkeypatch, lam, r):
    from snuffy_amd import functional as SF
    new, old = _spy(monkeypatch, ROW.single), _spy(monkeypatch, ROW.replaced)
    n = 3000
    net = _net(lam=lam, r=r)
    assert net.b_classifier.cfg.compute == "bf16"
    layer = net.b_classifier.encoder.layers[0]
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    x = torch.randn(n, D, generator=torch.Generator().manual_seed(77))
    _, logits_ref, p_ref, sels = orc.milnet_forward(x, sd, H, ACT, lam, r, 1, ReplayRNG(9))
    monkeypatch.setattr(SF, ROW.single_switch, False)
    with torch.no_grad():
        np.random.seed(9)
        _, y_off, a_off = net(x.to(DEV).unsqueeze(0))
        sel_off = tuple(None if t is None else t.clone() for t in layer.last_selection)
        assert (len(new), len(old)) == (0, 1)                                  # the call list of before: fp32 copies into the exact kernel
        del old[:]
        monkeypatch.setattr(SF, ROW.single_switch, True)
        np.random.seed(9)
        _, y_on, a_on = net(x.to(DEV).unsqueeze(0))
        assert (len(new), len(old)) == (1, 0)
    top, rnd = layer.last_selection
    assert torch.equal(top, sel_off[0]) and ((rnd is None and sel_off[1] is None) if r == 0 else torch.equal(rnd, sel_off[1]))
    assert np.array_equal((top if rnd is None else torch.cat((top, rnd))).cpu().numpy(), sels[0].numpy())
    dy, da = (y_on.cpu()[0] - logits_ref).abs().max().item(), (a_on[0].cpu() - p_ref).abs().max().item()
    print("single bag n=%d Lambda=%d against the oracle: |dlogit| %.3g  |dA| %.3g; against the switch-off forward: %.3g  %.3g"
          % (n, lam, dy, da, (y_on - y_off).abs().max().item(), (a_on - a_off).abs().max().item()))
    assert dy < ROW.ORACLE_TOL and da < ROW.ORACLE_TOL
    assert (a_on.sum(-1) - 1).abs().max().item() <= ROW.ROWSUM


@pytest.mark.filterwarnings("ignore:snuffy_amd. precision='bf16' on a stack:RuntimeWarning")
def test_deep_stack_keeps_the_fp32_class_route(monkeypatch, pack_on):
    """A stack deeper than one layer runs the fp32-class kernels whatever precision says: neither bf16 route is called, single bag or
    packed, and the call list is the one of before (the unfused pair per layer; packed: PACK_X3_DK256's varlen launches)."""
    from snuffy_amd import functional as SF
    monkeypatch.setattr(SF, ROW.single_switch, True)
    new, exact, pair = (_spy(monkeypatch, ROW.single), _spy(monkeypatch, "sparse_attn_fwd"),
                        _spy(monkeypatch, "sparse_attn_fwd_x3u"))
    bf_varlen, x3_varlen = _spy(monkeypatch, ROW.varlen), _spy(monkeypatch, "sparse_attn_fwd_x3_varlen")
    net = _net(depth=2)
    assert net.b_classifier.cfg.compute == "fp32"
    bags = _bags([1000, 1300], D, seed=3)
    with torch.no_grad():
        np.random.seed(9)
        net(bags[0])
        assert (len(new), len(exact), len(pair)) == (0, 0, 2 if not SF.X3_ATTN_DK256 else 0)
        np.random.seed(9)
        net.forward_bags(bags)
    assert not new and not exact and not bf_varlen
    from snuffy_amd import packed
    assert len(x3_varlen) == (2 if packed.PACK_X3_DK256 else 0)


def test_forward_bags_matches_per_bag_forwards(pack_on, monkeypatch):
    varlen, new, old = (_spy(monkeypatch, ROW.varlen), _spy(monkeypatch, ROW.single),
                        _spy(monkeypatch, ROW.replaced))
    from snuffy_amd import functional as SF
    monkeypatch.setattr(SF, ROW.single_switch, False)    # the per-bag loop is the route of before
    net = _net()
    bags = _bags(SIZES, D)
    with torch.no_grad():
        np.random.seed(11)
        ref, sel_ref = _loop(net, bags)
        assert (len(varlen), len(new), len(old)) == (0, 0, len(bags))
        np.random.seed(11)
        assert net._packable(bags)
        got = net.forward_bags(bags)
        assert (len(varlen), len(new), len(old)) == (1, 0, len(bags))   # one varlen launch per layer, no per-bag attention
        after_packed = np.random.rand()
        np.random.seed(11)
        [net(x) for x in bags]
        assert np.random.rand() == after_packed          # the numpy stream is left where the per-bag loop leaves it
    top, rnd = net.b_classifier.encoder.layers[0].last_selection_bags
    for b in range(len(bags)):                           # selections, random share included: bit-exact
        assert torch.equal(top[b], sel_ref[b][0][0]) and torch.equal(rnd[b], sel_ref[b][0][1]), b
        assert top[b].numel() == K_TOP
        _close(ROW, ref[b], got[b], SIZES[b])


def test_forward_bags_vs_oracle(pack_on):
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
        assert (got[b][2].sum(-1) - 1).abs().max().item() <= ROW.ROWSUM


def test_device_sampler_one_group_equals_the_loop(pack_on, device_sampler_on):
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


def test_device_sampler_mix_with_a_short_bag(pack_on, device_sampler_on):
    """A 600-row bag (shorter than Lambda: it selects all of its rows) next to the uniform group: pack_groups leaves it to the per-bag
    loop (a ragged group needs two bags, and 600 keys at this width are outside the ragged kernel), which runs after the group and
    draws from the next offset."""
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


def test_device_sampler_graph_replay_draws_fresh_rows(pack_on, device_sampler_on):
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
    calls = _spy(monkeypatch, ROW.varlen)
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
def test_fp32_is_routed_by_its_own_switch(monkeypatch, on):
    """precision="fp32" at this width packs behind PACK_X3_DK256 whatever PACK_DK256 says, on the fp32-class varlen kernel."""
    from snuffy_amd import packed
    monkeypatch.setattr(packed, ROW.pack_switch, on)
    bf_varlen, x3_varlen = _spy(monkeypatch, ROW.varlen), _spy(monkeypatch, "sparse_attn_fwd_x3_varlen")
    net = _net(precision="fp32")
    bags = _bags([1000, 1100], D, seed=13)
    for x3_on in (True, False):
        monkeypatch.setattr(packed, "PACK_X3_DK256", x3_on)
        del x3_varlen[:]
        with torch.no_grad():
            assert bool(net._pack_groups(bags)) is x3_on
            np.random.seed(11)
            net.forward_bags(bags)
        assert not bf_varlen and len(x3_varlen) == (1 if x3_on else 0)


def test_defaults_route_as_shipped(monkeypatch):
    """The routing that ships (profiles/attn_dk256.txt): the single bag keeps the fp32 copies into the exact kernel (MFMA_ATTN_DK256 off:
    the bf16 kernel is behind it at N = 8000), packed bags take the varlen launches of the new kernel (PACK_DK256 on: ahead of the loop at
    every row)."""
    from snuffy_amd import functional as SF
    from snuffy_amd import packed
    assert getattr(SF, ROW.single_switch) is ROW.SHIPPED[0] is False and getattr(packed, ROW.pack_switch) is ROW.SHIPPED[1] is True
    varlen, new, old = (_spy(monkeypatch, ROW.varlen), _spy(monkeypatch, ROW.single),
                        _spy(monkeypatch, ROW.replaced))
    sizes = ROW.SHIPPED_SIZES
    net = _net()
    bags = _bags(sizes, D, seed=13)
    with torch.no_grad():
        assert net._packable(bags) and net._pack_groups(bags) == [([0, 1, 2], False)]
        np.random.seed(11)
        got = net.forward_bags(bags)
        assert (len(varlen), len(new), len(old)) == (1, 0, 0)                  # one varlen launch set, no per-bag attention
        np.random.seed(11)
        ref = [net(x) for x in bags]
        assert (len(varlen), len(new), len(old)) == (1, 0, len(bags))          # the single bag: the exact kernel, as before
    for b, n in enumerate(sizes):
        _close(ROW, ref[b], got[b], n)
