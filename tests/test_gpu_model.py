"""Model-level parity on the GPU: snuffy_amd.snuffy.MILNet (HIP kernels through the C ABI) against
(a) the golden vectors captured from the reference, (b) the CPU oracle at the benchmark sizes."""
import math

import numpy as np
import pytest
import torch

from oracle import snuffy_oracle as orc
from tests.helpers import (TOL, ReplayRNG, build_amd_milnet, forced_sel, golden_files, load_case, rel_err, synth_state,
                           tol_for)

pytestmark = pytest.mark.gpu
DEV = "cuda"

def _record_error(fixture, precision, err_logits, err_a):
    """Measured errors per fixture -> gpurun_out/measured_f1.json (scratch; summarised in DESIGN.md)."""
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    os.makedirs(path, exist_ok=True)
    fn = os.path.join(path, "measured_f1.json")
    try:
        with open(fn) as f:
            rec = json.load(f)
    except (OSError, ValueError):
        rec = {}
    rec["%s/%s" % (fixture, precision)] = {"max_abs_logit_err": err_logits, "max_abs_A_err": err_a}
    with open(fn, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)


def load_net(z, sd, precision):
    N, D, h, lam, depth, seed = [int(v) for v in z["cfg"]]
    net = build_amd_milnet(D, h, str(z["act"]), lam, float(z["r"]), depth)
    net.load_state_dict(sd, strict=True)        # same key names as the reference's checkpoints
    return net.to(DEV).eval().configure(precision=precision, return_attention=True)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("path", golden_files("f1_"), ids=lambda p: p.split("/")[-1][:-4])
def test_f1_golden_forward(path, precision):
    z, sd = load_case(path)
    N, D, h, lam, depth, seed = [int(v) for v in z["cfg"]]
    net = load_net(z, sd, precision)
    x = torch.from_numpy(z["x"]).to(DEV)
    np.random.seed(seed)                         # the random share draws from the global numpy RNG like the reference
    with torch.no_grad():
        classes, logits, A = net(x)
    assert classes.shape == (1, N, 1) and logits.shape == (1, 1)
    np.testing.assert_allclose(classes.cpu().numpy(), z["classes"], rtol=0, atol=2e-5)
    fixture = path.split("/")[-1][:-4]
    err_l = float(np.abs(logits.cpu().numpy() - z["logits"]).max())
    if "A" in z.files:
        assert A.shape == z["A"].shape
        err_a = float(np.abs(A.cpu().numpy() - z["A"]).max())
    else:
        err_a = float(np.abs(A[:, :, torch.from_numpy(z["A_rows"]).to(DEV), :].cpu().numpy() - z["A_sub"]).max())
    _record_error(fixture, precision, err_l, err_a)
    assert err_l <= tol_for(precision, depth, fixture, "logits"), (fixture, precision, err_l)
    assert err_a <= tol_for(precision, depth, fixture, "A"), (fixture, precision, err_a)
    if precision == "fp32":                      # tight check too: the fp32 path is reference-class
        np.testing.assert_allclose(logits.cpu().numpy(), z["logits"], rtol=0, atol=3e-5)


@pytest.mark.parametrize("path", golden_files("f1_"), ids=lambda p: p.split("/")[-1][:-4])
def test_f1_selection_bit_exact_at_bclassifier_boundary(path):
    """With the reference's own critic scores as input, top-Lambda and the random draw are bit-identical."""
    z, sd = load_case(path)
    N, D, h, lam, depth, seed = [int(v) for v in z["cfg"]]
    net = load_net(z, sd, "fp32")
    x = torch.from_numpy(z["x"]).to(DEV)
    c = torch.from_numpy(z["classes"]).to(DEV)
    np.random.seed(seed)
    with torch.no_grad():
        logits, A = net.b_classifier(x, c)
    k1, k2 = orc.k_split(lam, float(z["r"]), N)
    for l, layer in enumerate(net.b_classifier.encoder.layers):
        top, rnd = layer.last_selection
        assert np.array_equal(top.cpu().numpy(), z["top"])
        if k2:
            assert np.array_equal(rnd.cpu().numpy(), z[f"rnd{l}"])
        else:
            assert rnd is None
    np.testing.assert_allclose(logits.cpu().numpy(), z["logits"], rtol=0, atol=3e-5)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("N,D,lam", [(8192, 384, 200), (32768, 768, 200), (100000, 768, 512)])
def test_benchmark_sizes_vs_oracle(N, D, lam, precision):
    """BASELINE.json configs A / B / C: full-size comparison against the CPU oracle (seconds on the host)."""
    h = 6
    net = synth_state(D, h, 1)
    net.b_classifier.encoder.layers[0].big_lambda = lam
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(1234)
    x = torch.randn(N, D, generator=g)
    classes_ref, logits_ref, p_ref, sels = orc.milnet_forward(x, sd, h, "relu", lam, 0.0, 1)
    net = net.to(DEV).eval().configure(precision=precision, return_attention=True)
    with torch.no_grad():
        classes, logits, A = net(x.to(DEV).unsqueeze(0))
        # selection is bit-exact when the scores are the oracle's
        _, A2 = net.b_classifier(x.to(DEV).unsqueeze(0), classes_ref.to(DEV).unsqueeze(0))
    top, _ = net.b_classifier.encoder.layers[0].last_selection
    assert np.array_equal(top.cpu().numpy(), sels[0].numpy())
    tol = TOL[precision]
    assert (classes.cpu()[0] - classes_ref).abs().max() < 2e-5
    assert (logits.cpu()[0] - logits_ref).abs().max() < tol
    rows = torch.arange(0, N, 97)
    assert (A2[0][:, rows.to(DEV), :].cpu() - p_ref[:, rows, :]).abs().max() < tol
    assert (A2.sum(-1) - 1).abs().max() < 1e-4
    # return_attention=False gives the same logits without the [1,h,N,K] tensor
    net.configure(return_attention=False)
    with torch.no_grad():
        _, logits2, A3 = net(x.to(DEV).unsqueeze(0))
    assert A3 is None and torch.equal(logits2, logits)


README_RECIPES = [   # reference README.md:609-669 ("Example Run for CAMELYON16"): h = 4 in all three
    (8192, 384, 4, 900, 0.7777777777777778),    # DINO from scratch: K = 200 top + 700 random, dk = 96 (rides padded to 128)
    (30000, 384, 4, 500, 0.5),                  # DINO with adapter: K = 250 + 250, dk = 96
    (8192, 768, 4, 500, 0.5),                   # MAE with adapter: dk = 192 (no MFMA form: exact fp32 attention kernel)
    (5000, 96, 2, 200, 0.25),                   # dk = 48 rides padded to 64
]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("N,D,h,lam,r", README_RECIPES)
def test_readme_recipes_vs_oracle(N, D, h, lam, r, precision, monkeypatch):
    """The reference's own published training recipes (h = 4: head widths 96 / 192, a random patch share): selection bit-exact
    (top AND the numpy draws), logits and attention inside the class against the oracle; the fp32-class path with padded heads equals
    the same forward on the exact fp32 attention kernel to rounding."""
    from snuffy_amd import functional as SF
    net = synth_state(D, h, 1)
    layer = net.b_classifier.encoder.layers[0]
    layer.big_lambda, layer.random_patch_share, layer.top_big_lambda_share = lam, r, 1.0 - r
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    x = torch.randn(N, D, generator=torch.Generator().manual_seed(77))
    x = x / x.norm(dim=1, keepdim=True)                                     # --l2normed_embeddings=1 (train.py:254-256)
    _, logits_ref, p_ref, sels = orc.milnet_forward(x, sd, h, "relu", lam, r, 1, ReplayRNG(9))
    net = net.to(DEV).eval().configure(precision=precision, return_attention=True)
    np.random.seed(9)
    with torch.no_grad():
        _, logits, A = net(x.to(DEV).unsqueeze(0))
    top, rnd = layer.last_selection
    k1 = math.ceil(lam * (1.0 - r))
    assert np.array_equal(torch.cat((top, rnd)).cpu().numpy(), sels[0].numpy()) and top.numel() == k1 and rnd.numel() == int(lam * r)
    tol = TOL[precision]
    assert (logits.cpu()[0] - logits_ref).abs().max() < tol
    rows = torch.arange(0, N, 53)
    assert (A[0][:, rows.to(DEV), :].cpu() - p_ref[:, rows, :]).abs().max() < tol
    assert (A.sum(-1) - 1).abs().max() < 1e-4
    if precision == "fp32":
        assert (logits.cpu()[0] - logits_ref).abs().max() < 3e-5            # fp32-class, as on the kernels' own head widths
        monkeypatch.setattr(SF, "FP32_ATTENTION", "exact")
        np.random.seed(9)
        with torch.no_grad():
            _, logits_e, A_e = net(x.to(DEV).unsqueeze(0))
        assert (logits_e - logits).abs().max() < 2e-5 and (A_e - A).abs().max() < 2e-5


def test_device_sampler_matches_host_twin_and_samples_uniformly():
    """csrc/sampler.hip against oracle/philox_ref.py: the keys bit for bit, the drawn rows exactly (descending key, ties by row);
    the draw avoids the excluded rows, has no duplicates, changes with the offset and the layer, and is uniform over the rest."""
    from oracle import philox_ref
    from snuffy_amd import ops
    n, k1, k2 = 5003, 200, 700
    top = torch.randperm(n, generator=torch.Generator().manual_seed(1))[:k1].to(DEV)
    smp = ops.DeviceSampler(torch.device(DEV), seed=1234567, offset=99)
    got = smp.draw(n, k2, top, layer=0).cpu().numpy()
    want = philox_ref.random_share_draw(n, k2, 1234567, 99, 0, top.cpu().numpy())
    assert np.array_equal(got, want)
    assert len(set(got.tolist())) == k2 and not (set(got.tolist()) & set(top.cpu().tolist()))
    assert not np.array_equal(got, smp.draw(n, k2, top, layer=1).cpu().numpy())          # another layer: another stream
    smp.advance()
    torch.cuda.synchronize()
    assert int(smp.state.cpu()[1]) == 100
    got2 = smp.draw(n, k2, top, layer=0).cpu().numpy()
    assert np.array_equal(got2, philox_ref.random_share_draw(n, k2, 1234567, 100, 0, top.cpu().numpy()))
    assert not np.array_equal(got, got2)
    # uniformity: 400 draws of 50 of 1000 rows -> every row's count ~ Binomial(400, 0.05); chi-square over the rows
    n, k2 = 1000, 50
    counts = np.zeros(n)
    smp = ops.DeviceSampler(torch.device(DEV), seed=7, offset=0)
    for _ in range(400):
        smp.advance()
        counts[smp.draw(n, k2, None).cpu().numpy()] += 1
    exp = 400 * k2 / n
    chi2 = ((counts - exp) ** 2 / (exp * (1 - k2 / n))).sum()
    assert 800 < chi2 < 1200, chi2                                     # ~ chi-square with 999 degrees of freedom (sd 45)
    with pytest.raises(ValueError):
        smp.draw(10, 11, None)


def test_device_sampler_model_fast_mode_and_graph_replay():
    """configure(sampler="device"): the random share comes from the device sampler (no host sync: numpy's stream is untouched), the
    model's outputs are those of the oracle given THAT selection, and a captured graph draws fresh rows on every replay."""
    N, D, h, lam, r = 6000, 384, 4, 500, 0.5
    net = synth_state(D, h, 1)
    layer = net.b_classifier.encoder.layers[0]
    layer.big_lambda, layer.random_patch_share, layer.top_big_lambda_share = lam, r, 1.0 - r
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    x = torch.randn(N, D, generator=torch.Generator().manual_seed(3))
    torch.manual_seed(11)
    net = net.to(DEV).eval().configure(precision="fp32", return_attention=True, sampler="device")
    np.random.seed(5)
    before = np.random.get_state()[1].copy()
    with torch.no_grad():
        _, logits, A = net(x.to(DEV).unsqueeze(0))
    assert np.array_equal(np.random.get_state()[1], before)             # the global numpy stream was not consumed
    top, rnd = layer.last_selection
    assert top.numel() == 250 and rnd.numel() == 250 and not (set(top.cpu().tolist()) & set(rnd.cpu().tolist()))

    # the oracle with the device's draw in place of numpy's (its top rows must be the oracle's own)
    _, logits_ref, p_ref, sels = orc.milnet_forward(x, sd, h, "relu", lam, r, 1, forced_sel=[torch.cat((top, rnd)).cpu()])
    assert np.array_equal(torch.cat((top, rnd)).cpu().numpy(), sels[0].numpy())
    assert (logits.cpu()[0] - logits_ref).abs().max() < 3e-5 and (A.cpu()[0] - p_ref).abs().max() < 1e-4
    # graph replay: captured once, fresh draws per replay (the offset advances on the device)
    net.configure(return_attention=False, graph_max_patches=1 << 20)
    xg = x.to(DEV).unsqueeze(0)
    outs, sels_seen = [], []
    with torch.no_grad():
        for _ in range(5):
            outs.append(net(xg)[1].clone())
    assert getattr(net, "_graphs", None), "the forward was not captured"
    assert len({float(o) for o in outs[2:]}) == 3                        # three replays, three different selections
    net.configure(sampler="reference")
    with pytest.raises(ValueError):
        net.configure(sampler="numpy")


def test_head_pad_table():
    from snuffy_amd import functional as SF
    assert [SF.head_pad(dk) for dk in (16, 32, 48, 64, 80, 96, 112, 128, 83, 192, 256)] == [64, 64, 64, 64, 128, 128, 128, 128, None, None, None]


def test_ragged_and_edge_bags():
    """N < Lambda (K = N), N == 1, depth 5, every activation -- through both precisions, vs the oracle."""
    for N, D, h, lam, r, depth, act in [(1, 64, 2, 10, 0.0, 1, "relu"), (7, 128, 2, 200, 0.0, 2, "gelu"),
                                        (300, 384, 6, 200, 0.25, 5, "selu"), (1025, 128, 1, 64, 0.5, 1, "leakyrelu")]:
        net = synth_state(D, h, depth, seed=N)
        for layer in net.b_classifier.encoder.layers:
            layer.big_lambda, layer.random_patch_share, layer.top_big_lambda_share = lam, r, 1.0 - r
            layer.feed_forward.activation_name = act
        sd = {k: v.clone() for k, v in net.state_dict().items()}
        x = torch.randn(N, D, generator=torch.Generator().manual_seed(N))
        _, logits_ref, p_ref, _ = orc.milnet_forward(x, sd, h, act, lam, r, depth, ReplayRNG(5))
        for precision in ("fp32", "bf16"):
            net = net.to(DEV).eval().configure(precision=precision)
            np.random.seed(5)
            with torch.no_grad():
                _, logits, A = net(x.to(DEV).unsqueeze(0))
            assert (logits.cpu()[0] - logits_ref).abs().max() < TOL[precision], (N, precision)
            assert (A.cpu()[0] - p_ref).abs().max() < TOL[precision], (N, precision)     # flat north-star gates, depth 5 included


def test_module_level_api_matches_reference_call_sites():
    """roi.py:177-194 style: i_classifier then b_classifier; Encoder / EncoderLayer / MHA callable on their own."""
    z, sd = load_case(golden_files("f1_n1000")[0])
    net = load_net(z, sd, "fp32")
    x = torch.from_numpy(z["x"]).to(DEV)
    with torch.no_grad():
        feats, c = net.i_classifier(x)
        logits, A = net.b_classifier(feats, c)
        zn, A2 = net.b_classifier.encoder(feats, c)
        lz, A3 = net.b_classifier.encoder.layers[0](feats, c)
        lin = net.b_classifier.linear
        pooled_logits = torch.nn.functional.linear(zn.mean(dim=1), lin.weight, lin.bias)
    assert feats.shape == x.shape and c.shape == (1, 1000, 1)
    np.testing.assert_allclose(logits.cpu().numpy(), z["logits"], rtol=0, atol=3e-5)
    assert zn.shape == x.shape and lz.shape == x.shape
    np.testing.assert_allclose(pooled_logits.cpu().numpy(), z["logits"], rtol=0, atol=3e-5)
    assert torch.equal(A, A2) and torch.equal(A, A3)
    with pytest.raises(IndexError):
        net(torch.cat([x, x]))                    # binary model: one bag per forward (as the reference)


@pytest.mark.parametrize("path", golden_files("f6_"), ids=lambda p: p.split("/")[-1][:-4])
def test_f6_multiclass_golden(path):
    """snuffy_multiclass (C = 2, B >= 1) against the reference goldens: per-class top-Lambda, unique, random share."""
    import copy

    from snuffy_amd import snuffy_multiclass as smc
    z, sd = load_case(path)
    B, N, D, h, lam, depth, seed = [int(v) for v in z["cfg"]]
    r = float(z["r"])
    attn = smc.MultiHeadedAttention(h, D)
    ff = smc.PositionwiseFeedForward(D, D * 4, "relu")
    net = smc.MILNet(smc.FCLayer(D, 2), smc.BClassifier(
        smc.Encoder(smc.EncoderLayer(D, copy.deepcopy(attn), copy.deepcopy(ff), 2, 0.0, lam, r), depth), 2, D))
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV).eval()
    x = torch.from_numpy(z["x"]).to(DEV)
    for precision in ("fp32", "bf16"):
        net.configure(precision=precision, return_attention=True)
        np.random.seed(seed)
        with torch.no_grad():
            classes, logits, A = net(x)
        tol = tol_for(precision, depth)
        np.testing.assert_allclose(classes.cpu().numpy(), z["classes"], rtol=0, atol=2e-5)
        np.testing.assert_allclose(logits.cpu().numpy(), z["logits"], rtol=0, atol=tol)
        assert tuple(A.shape) == tuple(z["A"].shape)
        np.testing.assert_allclose(A.cpu().numpy(), z["A"], rtol=0, atol=tol)
        if int(z["n_rnd"]):
            for l, layer in enumerate(net.b_classifier.encoder.layers):
                _, rnd = layer.last_selection
                got = rnd.cpu().numpy()
                want = np.stack([z[f"rnd{l * B + i}"] for i in range(B)])      # one np.random.choice call per row
                assert np.array_equal(got, want)


@pytest.mark.gpu
def test_fused_critic_layernorm_pass_changes_nothing():
    """MILNet.forward in bf16 hands the encoder the xhat produced by the critic pass (snf_critic_ln_f32).  Calling the two
    modules separately (the roi.py / reference call pattern) takes the unfused kernels: outputs must be bit-identical."""
    D, h, N = 384, 6, 3000
    net = synth_state(D, h, 1).to(DEV).eval().configure(precision="bf16", return_attention=True)
    x = torch.randn(1, N, D, generator=torch.Generator().manual_seed(5)).to(DEV)
    with torch.no_grad():
        classes, logits, A = net(x)
        feats, classes2 = net.i_classifier(x)
        logits2, A2 = net.b_classifier(feats, classes2)
    assert torch.equal(classes, classes2) and torch.equal(logits, logits2) and torch.equal(A, A2)
    # a stale offer must never be consumed: change the bag in place between the critic pass and the encoder
    from snuffy_amd import functional as SF
    with torch.no_grad():
        lin = net.i_classifier.fc[0]
        eps = net.b_classifier.encoder.layers[0].sublayer[0].norm.eps
        c3 = SF.critic_scores_with_xhat(x, lin.weight, lin.bias, eps, net.b_classifier.encoder.layers[0])
        x.mul_(2.0)                                           # bumps the version counter
        logits3, _ = net.b_classifier(x, c3)
        logits4, _ = net.b_classifier(x, c3)
    assert torch.equal(logits3, logits4)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_graph_replay_equals_eager(precision):
    """MILNet.configure(graph_max_patches=...): HIP-graph replay of the inference forward is the same kernels on the same
    data -- bit-identical outputs; small bags share one graph per shape (static input buffer), a large bag gets its own
    graph the second time the same tensor comes in; the random patch share (host RNG) keeps the eager path."""
    import torch
    from tests.helpers import build_amd_milnet
    dev = torch.device("cuda")
    torch.manual_seed(0)
    net = build_amd_milnet(384, 6, "relu", 200, 0.0, 1).to(dev).eval().configure(precision=precision, return_attention=False)
    g = torch.Generator().manual_seed(3)
    small = [torch.randn(1, n, 384, generator=g).to(dev) for n in (700, 700, 3000, 700)]
    large = torch.randn(1, 30000, 384, generator=g).to(dev)          # 46 MB: bound to its buffer, no copy
    with torch.no_grad():
        ref_s = [net(b) for b in small]
        ref_l = net(large)
        net.configure(graph_max_patches=100000)
        for _ in range(3):
            for b, r in zip(small, ref_s):
                out = net(b)
                assert torch.equal(out[0], r[0]) and torch.equal(out[1], r[1]) and out[2] is None
            out = net(large)
            assert torch.equal(out[0], ref_l[0]) and torch.equal(out[1], ref_l[1])
        assert len(net._graphs) == 3                                  # 700, 3000 (by shape) and the large buffer
        # the graphs share one memory pool, so what forward() hands out are copies: they survive later replays
        large2 = torch.randn(1, 31000, 384, generator=g).to(dev)
        held = net(large)
        for _ in range(2):
            net(large2)
            for b in small:
                net(b)
        assert torch.equal(held[0], ref_l[0]) and torch.equal(held[1], ref_l[1])
        large.mul_(0.5)                                               # same buffer, new contents: the graph reads it live
        net.configure(graph_max_patches=0)
        ref2 = net(large)
        net.configure(graph_max_patches=100000)
        net(large)
        out = net(large)
        assert torch.equal(out[1], ref2[1])
    # new weights invalidate the captured graphs (they hold the folded bf16 copies of the old ones)
    with torch.no_grad():
        for p_ in net.parameters():
            p_.mul_(1.01)
        net.configure(graph_max_patches=0)
        ref3 = net(small[0])
        net.configure(graph_max_patches=100000)
        net(small[0])
        out = net(small[0])
        assert torch.equal(out[1], ref3[1]) and torch.equal(out[0], ref3[0])
    rnd = build_amd_milnet(384, 6, "relu", 200, 0.5, 1).to(dev).eval().configure(precision=precision, graph_max_patches=100000)
    with torch.no_grad():
        rnd(small[0])
    assert len(rnd._graphs) == 0


@pytest.mark.gpu
def test_module_stays_picklable_and_copyable_after_forwards():
    """The per-layer caches (folded bf16 weights, split images of both formats, selector hand-over) hold plain tensors: a MILNet that
    has run forwards in both precisions can still be deep-copied and pickled whole (torch.save(model)), and the copy computes the same."""
    import copy
    import io
    net = build_amd_milnet(768, 6, "relu", 200, 0.0, 1).to(DEV).eval()
    x = torch.randn(1, 40000, 768, device=DEV)             # large enough for the fused selector and the one-pass GEMM
    with torch.no_grad():
        outs = {}
        for precision in ("fp32", "bf16"):
            net.configure(precision=precision, return_attention=False)
            outs[precision] = net(x)[1].clone()
        twin = copy.deepcopy(net)
        buf = io.BytesIO()
        torch.save(net, buf)
        buf.seek(0)
        loaded = torch.load(buf, weights_only=False)
        for m in (twin, loaded):
            for precision in ("fp32", "bf16"):
                m.configure(precision=precision, return_attention=False)
                assert torch.equal(m(x)[1], outs[precision]), precision


def test_invalidate_after_data_edit_drops_split_weight_caches():
    """the split-weight images cached on the parameters (_snf_img_cat / _snf_imgT_cat, keyed on data_ptr and _version) survive an
    edit through `.data`; MILNet.invalidate() is the documented remedy and must drop them: the forward after edit + invalidate
    equals the forward of a freshly built net with the edited weights."""
    from snuffy_amd import functional as SF
    D, h, N = 384, 6, 3000
    net = synth_state(D, h, 1).to(DEV).eval().configure(precision="fp32")
    x = torch.randn(1, N, D, generator=torch.Generator().manual_seed(3)).to(DEV)
    with torch.no_grad():
        net(x)                                             # populates every cache derived from the weights
        lk = net.b_classifier.encoder.layers[0].self_attn.linears[1]
        SF.split3_cached(lk.weight)                        # the training-path cache on the parameter itself
        assert hasattr(lk.weight, "_snf_img_cat")
        for p_ in net.parameters():
            if p_.dim() > 1:
                p_.data.mul_(1.25)                         # an EMA-style edit: same storage, same version counter
        net.invalidate()
        assert not hasattr(lk.weight, "_snf_img_cat")
        _, logits, _ = net(x)
        fresh = synth_state(D, h, 1).to(DEV).eval().configure(precision="fp32")
        fresh.load_state_dict(net.state_dict())
        _, logits_ref, _ = fresh(x)
    assert torch.allclose(logits, logits_ref, atol=1e-6), (logits, logits_ref)
