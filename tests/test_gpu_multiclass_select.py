"""The multiclass model's one-launch class-union selector (csrc/topk.hip: snf_multiclass_select_f32), the batched random keys
(csrc/sampler.hip: snf_random_share_keys_batched_f32) and EncoderLayer.select built on them.  Every comparison is exact."""
import copy
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def union_ref(c, k1):
    """CPU restatement (reference snuffy_multiclass.py:136-141): per row the ascending unique of the per-class top-k1 indices."""
    order = torch.sort(c, dim=1, descending=True, stable=True)[1][:, :k1, :].flatten(1)
    return [torch.unique(order[b]) for b in range(c.shape[0])]


def check_union(c, k1, want=None):
    from snuffy_amd import ops
    uniq, counts = ops.multiclass_select(c.to(DEV), k1)
    assert uniq.shape == (c.shape[0], c.shape[2] * k1) and uniq.dtype == torch.int64 and uniq.is_cuda
    assert counts.shape == (c.shape[0],) and counts.dtype == torch.int32 and counts.is_cuda
    uniq, counts = uniq.cpu(), counts.cpu()
    want = union_ref(c, k1) if want is None else want
    for b, w in enumerate(want):
        assert int(counts[b]) == w.numel(), (b, int(counts[b]), w.numel())
        assert torch.equal(uniq[b, :w.numel()], w.to(torch.int64)), b
    return counts


@pytest.mark.parametrize("shape", [(1, 100, 2, 10), (2, 60, 2, 5), (3, 1025, 3, 7), (1, 8193, 2, 200), (1, 70000, 2, 33),
                                   (2, 300, 1, 300), (1, 5000, 5, 800),
                                   (2, 64, 1365, 3), (1, 4100, 2, 2048)],      # the candidate list's last 24 words; k1 and C k1 at their caps
                                  ids=lambda s: "x".join(map(str, s)))
def test_union_matches_cpu_restatement(shape):
    B, N, C, k1 = shape
    c = torch.randn(B, N, C, generator=torch.Generator().manual_seed(N + k1))
    check_union(c, k1)


def test_union_special_inputs():
    from snuffy_amd import ops
    g = torch.Generator().manual_seed(4)
    N, k1 = 777, 31
    col = torch.randn(2, N, generator=g)
    # identical columns: every class selects the same rows
    counts = check_union(torch.stack((col, col, col), dim=2), k1)
    assert counts.tolist() == [k1, k1]
    # column 1 = -column 0: the highest and the lowest k1 rows, disjoint
    counts = check_union(torch.stack((col, -col), dim=2), k1)
    assert counts.tolist() == [2 * k1, 2 * k1]
    # all-equal scores: ties go to the lowest indices
    counts = check_union(torch.full((2, N, 2), 0.25), k1, want=[torch.arange(k1)] * 2)
    assert counts.tolist() == [k1, k1]
    # +-0, +-inf and NaN in a column: the project's own order, the one ops.topk gives
    sp = torch.randn(1, 400, 2, generator=g)
    sp[0, 3::17, 0] = 0.0
    sp[0, 5::19, 0] = -0.0
    sp[0, 7::23, 0] = float("inf")
    sp[0, 11::29, 0] = float("-inf")
    sp[0, 13::31, 0] = float("nan")
    for k in (9, 40, 395):
        spd = sp.to(DEV)
        cols = [ops.topk(spd[0, :, cc], k).cpu() for cc in range(2)]
        check_union(sp, k, want=[torch.unique(torch.cat(cols))])


def test_domain_is_refused_with_a_message_and_the_old_path_still_answers():
    from snuffy_amd import _ffi, ops
    from snuffy_amd import snuffy_multiclass as smc
    assert ops.multiclass_select_supported(1, 5000, 2, 2048) and not ops.multiclass_select_supported(1, 5000, 2, 2049)
    lib = _ffi.load()
    for (B, N, C, k1) in [(1, 5000, 17, 241), (1, 20, 2, 21)]:          # C * k1 = 4097; k1 > N
        assert not ops.multiclass_select_supported(B, N, C, k1)
        c = torch.randn(B, N, C, generator=torch.Generator().manual_seed(1)).to(DEV)
        with pytest.raises(_ffi.SnuffyHipError, match="outside the kernel"):
            ops.multiclass_select(c, k1)
        uniq = torch.empty(B, C * k1, dtype=torch.int64, device=DEV)
        counts = torch.empty(B, dtype=torch.int32, device=DEV)
        rc = lib.snf_multiclass_select_f32(ctypes.c_void_p(c.data_ptr()), B, N, C, k1, ctypes.c_void_p(uniq.data_ptr()),
                                           ctypes.c_void_p(counts.data_ptr()), None)
        assert rc in (_ffi.SNF_EUNSUPPORTED, _ffi.SNF_EINVAL)
        assert b"snf_multiclass_select_f32" in lib.snf_last_error()
    # the model at C * k1 = 4097 keeps the per-class path, same answer as select_unfused
    layer = make_layer(64, 2, 17, 241, 0.0).to(DEV)
    c = torch.randn(1, 5000, 17, generator=torch.Generator().manual_seed(2)).to(DEV)
    np.random.seed(3)
    got = layer.select(c)
    np.random.seed(3)
    want = layer.select_unfused(c)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert smc.FUSED_SELECT is True


def make_layer(D, h, C, lam, r):
    from snuffy_amd import snuffy_multiclass as smc
    return smc.EncoderLayer(D, smc.MultiHeadedAttention(h, D), smc.PositionwiseFeedForward(D, 4 * D, "relu"), C, 0.0, lam, r)


@pytest.mark.parametrize("case", [(2, 60, 2, 6, 0.3), (1, 400, 2, 40, 0.5)], ids=lambda s: "x".join(map(str, s)))
def test_select_is_select_unfused_bit_for_bit(case):
    """Same (topk, rnd) and the same position of numpy's global stream afterwards."""
    B, N, C, lam, r = case
    layer = make_layer(64, 2, C, lam, r).to(DEV)
    c = torch.randn(B, N, C, generator=torch.Generator().manual_seed(N)).to(DEV)
    for s in (0, 7):
        np.random.seed(s)
        t0, r0 = layer.select_unfused(c)
        st0 = np.random.get_state()
        np.random.seed(s)
        t1, r1 = layer.select(c)
        st1 = np.random.get_state()
        assert t0.shape[1] > 0 and torch.equal(t0, t1) and torch.equal(r0, r1)
        assert st0[0] == st1[0] and np.array_equal(st0[1], st1[1]) and st0[2:] == st1[2:]


def test_device_sampler_draws_the_host_twins_rows():
    """set_sampler("device"): row b's random rows are the Philox draw of stream layer + 64 b outside ALL of the row's unique indices,
    numpy's stream is not consumed, and every forward draws anew."""
    from oracle import philox_ref
    from snuffy_amd import ops
    from snuffy_amd import snuffy_multiclass as smc
    B, N, C, D, h, lam, r, depth = 3, 500, 2, 64, 2, 30, 0.4, 2
    seed, offset = 424242, 1000
    layer = make_layer(D, h, C, lam, r)
    net = smc.MILNet(smc.FCLayer(D, C), smc.BClassifier(smc.Encoder(layer, depth), C, D)).to(DEV).eval()
    net.configure(precision="fp32", return_attention=False, sampler="device")
    cfg = net.b_classifier.cfg
    cfg._device_sampler = ops.DeviceSampler(torch.device(DEV, torch.cuda.current_device()), seed=seed, offset=offset)
    x = torch.randn(B, N, D, generator=torch.Generator().manual_seed(5)).to(DEV)
    k1 = math.ceil(lam * (1.0 - r))
    np.random.seed(9)
    before = np.random.get_state()[1].copy()
    seen = []
    for fwd in (1, 2):
        with torch.no_grad():
            classes, _, _ = net(x)
        assert cfg._device_sampler.seed == seed                               # the sampler given above is the one in use
        uniq = union_ref(classes.cpu(), k1)
        ref_dim = min(u.numel() for u in uniq)
        ref_dim = min(ref_dim, N - ref_dim)
        for li, l in enumerate(net.b_classifier.encoder.layers):
            topk, rnd = l.last_selection
            assert rnd.shape == (B, ref_dim) and ref_dim > 0
            for b in range(B):
                want = philox_ref.random_share_draw(N, ref_dim, seed, offset + fwd, li + 64 * b, exclude=uniq[b].numpy())
                assert np.array_equal(rnd[b].cpu().numpy(), want), (fwd, li, b)
                assert torch.equal(topk[b].cpu(), uniq[b][:ref_dim])
        seen.append(net.b_classifier.encoder.layers[0].last_selection[1].cpu())
    assert np.array_equal(np.random.get_state()[1], before)                   # the global numpy stream was not consumed
    assert not torch.equal(seen[0], seen[1])                                  # two forwards draw different rows
    # a layer called on its own advances the sampler itself
    with torch.no_grad():
        net.b_classifier.encoder.layers[0](x, classes, 0)
    torch.cuda.synchronize()
    assert int(cfg._device_sampler.state.cpu()[1]) == offset + 3
    assert copy.deepcopy(net).b_classifier.cfg._device_sampler is None
