"""Packed (varlen) inference above one key chunk and at padded head widths (the README recipes: D = 384, h = 4, Lambda = 900 / 500).
Kernel level: the key-chunked varlen launches of both families against the single-bag key-chunked entry points (same P and lse bit for
bit, O up to the fp32 order of the partial sums), independent of the batch composition bit for bit, and against fp64.  Model level:
MILNet.forward_bags with packed.PACK_KEY_CHUNKS on against the per-bag forwards and the CPU oracle, through a captured graph, and the
routing of before with the switch off."""
import numpy as np
import pytest
import torch

from oracle import snuffy_oracle as orc
from tests.attn_widths import _bags, _fp64_reference, _packed, _sizes
from tests.helpers import build_amd_milnet

pytestmark = pytest.mark.gpu
DEV = "cuda"

LENGTHS = [None, 1000, 777, 2048, 4100]          # None: a bag of exactly k rows; a tile tail; directly stored bags (<= 1024); reduced bags
SHAPES = [(768, 6, 225),                          # smallest chunked case: chunks 113 / 112 (bf16), 116 / 109 (fp32-class)
          (768, 6, 448),                          # 2 x 224: 7 key blocks
          (512, 4, 500),                          # 3 chunks
          (384, 6, 257),                          # dk = 64; bf16 chunks 129 / 128: different key-block counts
          (512, 4, 900)]                          # 5 chunks


def _check_family(fam, d, h, k, need_attn):
    from snuffy_amd import ops
    sizes = _sizes(k, LENGTHS)
    pk = _packed(sizes)
    g = torch.Generator().manual_seed(1 if fam == "bf16" else 2)
    qv = torch.randn(pk.total, 2 * d, generator=g).to(DEV)
    kp = (torch.randn(pk.bags * k, d, generator=g) * 0.5).to(DEV)
    if fam == "bf16":
        qv, kp = qv.to(torch.bfloat16), kp.to(torch.bfloat16)
        varlen = ops.sparse_attn_fwd_mfma_varlen

        def single(qb, vb, kb, n):
            return ops.sparse_attn_fwd_mfma(qb, vb, kb, n, h, need_attn=need_attn, need_lse=need_attn)
    else:
        varlen = ops.sparse_attn_fwd_x3_varlen

        def single(qb, vb, kb, n):
            return ops.sparse_attn_fwd_x3(qb, vb, kb, h, need_attn=need_attn, need_lse=need_attn)
    assert not ops.varlen_attn_supported(fam, k, d // h) and ops.varlen_attn_chunks_supported(fam, k, d // h)
    q, v = qv[:, :d], qv[:, d:]
    out, attn, lse = varlen(q, v, kp, pk, k, h, need_attn=need_attn, need_lse=need_attn)
    assert out.shape == (pk.bags * k, d)
    for b, n in enumerate(sizes):
        lo = int(pk.host[b])
        qb, kb = qv[lo:lo + n], kp[b * k:(b + 1) * k]
        o1, a1, l1 = single(qb[:, :d], qb[:, d:], kb, n)
        err, ref = (out[b * k:(b + 1) * k] - o1).abs().max().item(), o1.abs().max().item()
        print("%s d=%d h=%d k=%d bag %d n=%d: |out - single| / max|out| = %.3g" % (fam, d, h, k, b, n, err / ref))
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
    # and against fp64 on one bag (the kernels agree with each other; this pins them to the definition)
    b = 1
    lo, n = int(pk.host[b]), sizes[b]
    ref = _fp64_reference((fam, d, h, k), qv[lo:lo + n, :d], qv[lo:lo + n, d:], kp[b * k:(b + 1) * k], h)
    err = (out[b * k:(b + 1) * k].double() - ref).abs().max().item() / ref.abs().max().item()
    print("%s d=%d h=%d k=%d: relative error against fp64 %.3g" % (fam, d, h, k, err))
    assert err < (1e-2 if fam == "bf16" else 2e-5), err


@pytest.mark.parametrize("d,h,k", SHAPES)
@pytest.mark.parametrize("need_attn", [False, True])
def test_attention_bf16_varlen_chunks_vs_per_bag_and_composition_independent(d, h, k, need_attn):
    _check_family("bf16", d, h, k, need_attn)


@pytest.mark.parametrize("d,h,k", SHAPES)
@pytest.mark.parametrize("need_attn", [False, True])
def test_attention_x3_varlen_chunks_vs_per_bag_and_composition_independent(d, h, k, need_attn):
    _check_family("fp32", d, h, k, need_attn)


# ---- model level ----------------------------------------------------------------------------------------------------------------------
def _net(d, h, lam, r, depth, precision, seed=0):
    torch.manual_seed(seed)
    net = build_amd_milnet(d, h, "relu", lam, r, depth).to(DEV).eval()
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() > 1:
                torch.nn.init.xavier_uniform_(p)
    net.configure(precision=precision, return_attention=True)
    return net


@pytest.fixture
def chunks_on(monkeypatch):
    from snuffy_amd import packed
    monkeypatch.setattr(packed, "PACK_KEY_CHUNKS", True)           # the switch under test, whatever its shipped default


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("lam,r", [(500, 0.5), (900, 0.0)])
def test_forward_bags_of_the_readme_recipes_matches_per_bag_forwards(chunks_on, precision, lam, r):
    d, h = 384, 4                                                    # dk = 96, padded to 128 on the packed path
    sizes = [lam, 1000, 1333, 4100, 2048]
    net = _net(d, h, lam, r, 1, precision)
    bags = _bags(sizes, d)
    with torch.no_grad():
        np.random.seed(11)
        ref, sel_ref = [], []
        for x in bags:
            ref.append(net(x))
            sel_ref.append([tuple(None if t is None else t.clone() for t in l.last_selection) for l in net.b_classifier.encoder.layers])
        np.random.seed(11)
        assert net._packable(bags)
        got = net.forward_bags(bags)
        after_packed = np.random.rand()
        np.random.seed(11)
        [net(x) for x in bags]
        assert np.random.rand() == after_packed          # the numpy stream is left where the per-bag loop leaves it
    for li, layer in enumerate(net.b_classifier.encoder.layers):       # selections, random share included: bit-exact
        top, rnd = layer.last_selection_bags
        for b in range(len(bags)):
            assert torch.equal(top[b], sel_ref[b][li][0])
            assert (rnd is None and sel_ref[b][li][1] is None) or torch.equal(rnd[b], sel_ref[b][li][1])
    tol_logit, tol_a, tol_sum = (2e-5, 2e-5, 1e-4) if precision == "fp32" else (2e-2, 2e-2, 1e-3)
    for b, ((c0, y0, a0), (c1, y1, a1)) in enumerate(zip(ref, got)):
        assert c1.shape == c0.shape and y1.shape == y0.shape and a1.shape == a0.shape == (1, h, sizes[b], lam)
        assert torch.equal(c0, c1)                       # critic scores: same kernel, row-wise
        dy, da = (y0 - y1).abs().max().item(), (a0 - a1).abs().max().item()
        ds = (a1.sum(-1) - 1).abs().max().item()
        print("%s lam=%d bag %d: |dlogit| %.3g  |dA| %.3g  |rowsum - 1| %.3g" % (precision, lam, b, dy, da, ds))
        assert dy <= tol_logit * max(1.0, y0.abs().max().item()), (b, y0, y1)
        assert da <= tol_a, b
        # A's entries are ~1 / Lambda: only the row sum notices a chunk normalised by the wrong statistics
        assert ds <= tol_sum, b


@pytest.mark.parametrize("precision,tol", [("fp32", 1e-3), ("bf16", 2e-2)])
def test_forward_bags_of_a_readme_recipe_vs_oracle(chunks_on, precision, tol):
    d, h, lam = 384, 4, 500
    sizes = [1000, 1500, 600]
    net = _net(d, h, lam, 0.0, 1, precision)
    bags = _bags(sizes, d, seed=9)
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        assert net._packable(bags)
        got = net.forward_bags(bags)
    top, _ = net.b_classifier.encoder.layers[0].last_selection_bags
    for b, x in enumerate(bags):
        classes, logits, attn, sels = orc.milnet_forward(x[0].cpu(), sd, h, "relu", lam, 0.0, 1)
        assert np.array_equal(sels[0].numpy(), top[b].cpu().numpy())                   # bit-exact top-Lambda indices per bag
        dy, da = (got[b][1][0].cpu() - logits).abs().max().item(), (got[b][2][0].cpu() - attn).abs().max().item()
        print("%s bag %d against the oracle: |dlogit| %.3g  |dA| %.3g" % (precision, b, dy, da))
        assert dy <= tol * max(1.0, logits.abs().max().item())
        assert da <= tol


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_forward_bags_of_a_readme_recipe_through_a_graph(chunks_on, precision):
    sizes = [1000, 600, 2048]
    net = _net(384, 4, 500, 0.0, 1, precision)
    bags = _bags(sizes, 384, seed=13)
    with torch.no_grad():
        assert net._packable(bags)
        got = net.forward_bags(bags)
        net.configure(graph_max_patches=1 << 16)
        net.forward_bags(bags)                        # first sight of a composition: eager (remembered)
        got_graph = net.forward_bags(bags)            # second: captured and replayed
        got_graph2 = net.forward_bags(bags)           # third: replay only
        assert sum(1 for k in net._graphs if k and k[0] == "bags") == 1
        net.configure(graph_max_patches=0)
    for (c1, y1, a1), (c2, y2, a2), (c3, y3, a3) in zip(got, got_graph, got_graph2):
        assert torch.equal(c1, c2) and torch.equal(y1, y2) and torch.equal(a1, a2)      # graph replay == eager issue, bit for bit
        assert torch.equal(c1, c3) and torch.equal(y1, y3) and torch.equal(a1, a3)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_switch_off_keeps_the_per_bag_loop(monkeypatch, precision):
    from snuffy_amd import packed
    monkeypatch.setattr(packed, "PACK_KEY_CHUNKS", False)
    net = _net(384, 4, 500, 0.0, 1, precision)
    bags = _bags([1000, 600, 2048], 384, seed=13)
    with torch.no_grad():
        assert not net._packable(bags) and net._pack_groups(bags) is None
        got = net.forward_bags(bags)
        ref = [net(x) for x in bags]
    for (c0, y0, a0), (c1, y1, a1) in zip(ref, got):
        assert torch.equal(c0, c1) and torch.equal(y0, y1) and torch.equal(a0, a1)
