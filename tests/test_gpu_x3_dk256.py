"""Fused fp32-class (split-bf16 x 3) sparse attention at head width 256 (the README's SimCLR ResNet-18 recipe: D = 512, h = 2,
Lambda = 900 as 200 + 700, gelu), single bag and packed.
Kernel level (D = 512, h = 2: the model width of the recipe): the single-bag entry point against the fp64 oracle inside the fp32-class
family's bounds and against the unfused pair it replaces; the varlen launches against the single-bag entry point (same P and lse bit for
bit, O up to the fp32 order of the partial sums), independent of the batch composition bit for bit, against fp64, and bit-identical on a
repeat.
Model level: the single-bag forward behind functional.X3_ATTN_DK256 at depth 1 and on a depth-2 stack, MILNet.forward_bags behind
packed.PACK_X3_DK256 against the per-bag forwards and the CPU oracle, with the device sampler (one group, a mix with a short bag), and
the routing that ships with both switches at their defaults."""
import numpy as np
import pytest
import torch

from oracle import snuffy_oracle as orc
from tests.attn_widths import (OFFSET, X3_256 as ROW, _bags, _close, _fp64_reference, _loop, _offset, _packed, _place_sampler, _sizes,
                               _spy, device_sampler_on, op, pack_on)  # noqa: F401  (fixtures)
from tests.helpers import ReplayRNG, _ops, build_amd_milnet, rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture
def row():
    return ROW
DEV = "cuda"

D_K, H_K, DK = ROW.D_K, ROW.H_K, ROW.dk


# ---- single bag -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,h", ROW.SHAPES)
def test_sparse_attn_x3_dk256_fp32_class(n, k, h):
    """Bounds: those of test_sparse_attn_x3_fp32_class / test_sparse_attn_x3u_fp32_class, which the unfused pair holds at dk = 256
    (P 1e-5, O 2e-5 of its scale up to 256 keys and 4e-5 above, lse 3e-5, row sums 1e-5, all against fp64); against the unfused pair P
    within the sum of the two P bounds."""
    ops = _ops()
    dk = DK
    g = torch.Generator().manual_seed(ROW.seed(n, k, h))
    d = h * dk
    q, kp, v = torch.randn(n, d, generator=g), torch.randn(k, d, generator=g), torch.randn(n, d, generator=g)
    o_ref, p_ref = orc.sparse_attention(q.double(), kp.double(), v.double(), h)
    assert op(ROW, "single_supported")(k) and not ops.x3_attn_supported(k, dk)
    qd, kd, vd = q.to(DEV), kp.to(DEV), v.to(DEV)
    o, attn, lse = op(ROW, "single")(qd, vd, kd, h, need_attn=True, need_lse=True)
    s_ref = (q.double().view(n, h, dk).transpose(0, 1) @ kp.double().view(k, h, dk).transpose(0, 1).transpose(1, 2)) / dk ** 0.5
    e_p = (attn.cpu().double() - p_ref).abs().max().item()
    e_o = rel_err(o.cpu(), o_ref)
    e_l = (lse.cpu().double() - torch.logsumexp(s_ref, dim=-1)).abs().max().item()
    e_s = (attn.sum(-1) - 1).abs().max().item()
    print("x3 dk=256 n=%d k=%d h=%d: |dP| %.3g  O rel %.3g  |dlse| %.3g  |rowsum - 1| %.3g" % (n, k, h, e_p, e_o, e_l, e_s))
    assert e_p < 1e-5
    assert e_o < ROW.O_FP64[k > 256]
    assert e_l < 3e-5
    assert e_s < 1e-5
    # the unfused pair on the same operands
    _, a_u, _ = op(ROW, "replaced")(qd, kd, vd, h, need_attn=True)
    e_u = (attn - a_u).abs().max().item()
    print("x3 dk=256 n=%d k=%d h=%d: |P - P(x3u)| %.3g" % (n, k, h, e_u))
    assert e_u < 2e-5
    # the same O without the A output; a repeat call is bit-identical
    o2, a2, l2 = op(ROW, "single")(qd, vd, kd, h)
    assert a2 is None and l2 is None and torch.equal(o2, o)
    o3, a3, l3 = op(ROW, "single")(qd, vd, kd, h, need_attn=True, need_lse=True)
    assert torch.equal(o3, o) and torch.equal(a3, attn) and torch.equal(l3, lse)
    # the halves of a fused [Q | V] projection output, used in place (row pitch 2 d)
    qv = torch.cat([q, v], dim=1).to(DEV)
    o4, a4, _ = op(ROW, "single")(qv[:, :d], qv[:, d:], kd, h, need_attn=True)
    assert torch.equal(o4, o) and torch.equal(a4, attn)


def test_sparse_attn_x3_dk256_refuses_other_shapes():
    from snuffy_amd import SnuffyHipError
    ops = _ops()
    z = lambda *s: torch.zeros(*s, device=DEV)                                  # noqa: E731
    with pytest.raises((SnuffyHipError, ValueError)):
        op(ROW, "single")(z(64, D_K), z(64, D_K), z(1025, D_K), 2)
    with pytest.raises((SnuffyHipError, ValueError)):
        op(ROW, "single")(z(64, 256), z(64, 256), z(8, 256), 2)     # dk = 128


# ---- varlen -----------------------------------------------------------------------------------------------------------------------------
KEYS = ROW.KEYS


@pytest.mark.parametrize("k", KEYS)
@pytest.mark.parametrize("need_attn", [False, True])
def test_attention_varlen_x3_dk256_vs_per_bag_and_composition_independent(k, need_attn):
    ops = _ops()
    d, h = D_K, H_K
    sizes = _sizes(k)
    pk = _packed(sizes)
    g = torch.Generator().manual_seed(1)
    qv = torch.randn(pk.total, 2 * d, generator=g).to(DEV)
    kp = (torch.randn(pk.bags * k, d, generator=g) * 0.5).to(DEV)
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
        print("x3 dk=256 k=%d bag %d n=%d: |out - single| / max|out| = %.3g" % (k, b, n, err / ref))
        # the single-bag entry point spreads a small bag over more workgroups (one tile each; a packed bag takes up to 32 tiles per
        # workgroup): same P, O up to the fp32 order of the partial sums
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
    err = rel_err(out[b * k:(b + 1) * k].cpu(), ref)
    print("x3 dk=256 k=%d: relative error against fp64 %.3g" % (k, err))
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


def _net(sampler=None, return_attention=True, seed=0, depth=1, precision="fp32"):
    torch.manual_seed(seed)
    net = build_amd_milnet(D, H, ACT, LAM, R, depth).to(DEV).eval()
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() > 1:
                torch.nn.init.xavier_uniform_(p)
    if sampler is None:
        net.configure(precision=precision, return_attention=return_attention)
    else:
        net.configure(precision=precision, return_attention=return_attention, sampler=sampler)
    return net


@pytest.mark.parametrize("depth,precision", [(1, "fp32"),
                                             (2, "bf16")])   # a stack runs the fp32-class kernels whatever precision says: roi.py's route
@pytest.mark.filterwarnings("ignore:snuffy_amd. precision='bf16' on a stack:RuntimeWarning")
def test_single_bag_routing_and_oracle(monkeypatch, depth, precision):
    from snuffy_amd import functional as SF
    new, old = _spy(monkeypatch, ROW.single), _spy(monkeypatch, ROW.replaced)
    n = 3000
    net = _net(depth=depth, precision=precision)
    assert net.b_classifier.cfg.compute == "fp32"
    layers = net.b_classifier.encoder.layers
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    x = torch.randn(n, D, generator=torch.Generator().manual_seed(77))
    _, logits_ref, p_ref, sels = orc.milnet_forward(x, sd, H, ACT, LAM, R, depth, ReplayRNG(9))
    monkeypatch.setattr(SF, ROW.single_switch, False)
    with torch.no_grad():
        np.random.seed(9)
        _, y_off, a_off = net(x.to(DEV).unsqueeze(0))
        sel_off = [tuple(t.clone() for t in l.last_selection) for l in layers]
        assert (len(new), len(old)) == (0, depth)                              # the call list of before: the unfused pair only
        monkeypatch.setattr(SF, ROW.single_switch, True)
        np.random.seed(9)
        _, y_on, a_on = net(x.to(DEV).unsqueeze(0))
        assert (len(new), len(old)) == (depth, depth)
    for li, layer in enumerate(layers):
        top, rnd = layer.last_selection
        assert torch.equal(top, sel_off[li][0]) and torch.equal(rnd, sel_off[li][1])
        assert np.array_equal(torch.cat((top, rnd)).cpu().numpy(), sels[li].numpy()) and top.numel() == K_TOP
    dy, da = (y_on.cpu()[0] - logits_ref).abs().max().item(), (a_on[0].cpu() - p_ref).abs().max().item()
    print("single bag n=%d depth %d against the oracle: |dlogit| %.3g  |dA| %.3g; against the switch-off forward: %.3g  %.3g"
          % (n, depth, dy, da, (y_on - y_off).abs().max().item(), (a_on - a_off).abs().max().item()))
    assert dy < ROW.ORACLE_TOL and da < ROW.ORACLE_TOL
    assert (a_on.sum(-1) - 1).abs().max().item() <= ROW.ROWSUM


@pytest.mark.parametrize("depth", [1, 2])              # 2: a stack, as roi.py's model is (every layer packs)
def test_forward_bags_matches_per_bag_forwards(pack_on, monkeypatch, depth):
    varlen, new, old = (_spy(monkeypatch, ROW.varlen), _spy(monkeypatch, ROW.single),
                        _spy(monkeypatch, ROW.replaced))
    from snuffy_amd import functional as SF
    monkeypatch.setattr(SF, ROW.single_switch, False)      # the per-bag loop is the route of before
    net = _net(depth=depth)
    bags = _bags(SIZES, D)
    with torch.no_grad():
        np.random.seed(11)
        ref, sel_ref = _loop(net, bags)
        assert (len(varlen), len(new), len(old)) == (0, 0, depth * len(bags))
        np.random.seed(11)
        assert net._packable(bags)
        got = net.forward_bags(bags)
        assert (len(varlen), len(new), len(old)) == (depth, 0, depth * len(bags))   # one varlen launch per layer, no per-bag attention
        after_packed = np.random.rand()
        np.random.seed(11)
        [net(x) for x in bags]
        assert np.random.rand() == after_packed          # the numpy stream is left where the per-bag loop leaves it
    for li, layer in enumerate(net.b_classifier.encoder.layers):
        top, rnd = layer.last_selection_bags
        for b in range(len(bags)):                       # selections, random share included: bit-exact
            assert torch.equal(top[b], sel_ref[b][li][0]) and torch.equal(rnd[b], sel_ref[b][li][1]), (li, b)
    for b in range(len(bags)):
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
        assert dy <= ROW.Y_TOL and da <= ROW.A_TOL


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
            assert (y0 - y1).abs().max().item() <= ROW.Y_TOL, i
            assert (a0 - a1).abs().max().item() <= ROW.A_TOL, i


def test_defaults_route_as_shipped(monkeypatch):
    """The routing that ships (profiles/x3_dk256.txt): the single bag keeps the unfused pair (X3_ATTN_DK256 off: the fused kernel is
    behind it at every row), packed bags take the varlen launches of the new kernel (PACK_X3_DK256 on: ahead of the loop at every row)."""
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
        assert (len(varlen), len(new), len(old)) == (1, 0, len(bags))          # the single bag: the unfused pair, as before
    for b, n in enumerate(sizes):
        _close(ROW, ref[b], got[b], n)
