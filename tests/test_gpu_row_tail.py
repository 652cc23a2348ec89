"""Row tail of the weight-gradient contraction on the GPU: snf_gemm_tn_f32 for bag lengths that are no multiple of its 32-row step,
in all three operand layouts (one bf16 product, plane images [hi | hi | lo], interleaved hl images), and the training chains that now
take such bags."""
import numpy as np
import pytest
import torch

from tests.helpers import build_amd_milnet

pytestmark = pytest.mark.gpu
DEV = "cuda"

# n % 32 = 1, 1, 3, 5, 13, 31: the cut falls inside the staging rows of wave 0 (rows 0 - 3), 1 (4 - 7), 3 (12 - 15) and behind the last
# wave's (row 30), so every wave stages a whole, a half and an empty piece at least once
LENGTHS = (1025, 2049, 4099, 16389, 32749, 32767)
SHAPES = ((520, 264), (768, 3072), (1536, 768))
HL_SHAPES = ((512, 288), (768, 3072), (1536, 768))          # hl images come in 32-column groups


def _operands(n, p, q, layout, seed=0):
    """(a image, b image, gemm_tn keyword arguments, fp64 reference) of two random matrices in one of the three layouts."""
    from snuffy_amd import ops
    g = torch.Generator().manual_seed(n + p + q + seed)
    a = torch.randn(n, p, generator=g).to(DEV)
    b = torch.randn(n, q, generator=g).to(DEV)
    if layout == "bf16":
        a_img, b_img = a.to(torch.bfloat16), b.to(torch.bfloat16)
        return a_img, b_img, {}, a_img.double().t() @ b_img.double()
    if layout == "x3":
        return ops.split3_rows(a), ops.split3_rows(b), dict(a_planes=(p, 2 * p), b_planes=(q, 2 * q)), a.double().t() @ b.double()
    return ops.split_hl_rows(a), ops.split_hl_rows(b), dict(hl=True), a.double().t() @ b.double()


def _tol(layout):
    return 2e-6 if layout == "bf16" else 2e-5               # test_gemm_tn_weight_gradient_contraction / test_gemm_tn_interleaved_images


def _cases():
    for layout in ("bf16", "x3", "hl"):
        for n in LENGTHS:
            for p, q in (HL_SHAPES if layout == "hl" else SHAPES):
                yield pytest.param(n, p, q, layout, id="%s-%d-%dx%d" % (layout, n, p, q))


@pytest.mark.parametrize("n,p,q,layout", list(_cases()))
def test_gemm_tn_row_tail_against_fp64_and_the_zero_padded_bag(n, p, q, layout):
    """ops.gemm_tn at a bag length off the 32-row grid: against fp64 of the same operands, bit-identical run to run, and bit-identical
    to the contraction of the same images padded with zero rows to the next multiple of 32 (as many steps, hence the same row parts
    and the same summation order; the padded rows add exact zeros)."""
    from snuffy_amd import ops
    a_img, b_img, kw, ref = _operands(n, p, q, layout)
    out = ops.gemm_tn(a_img, b_img, p, q, **kw)
    err, scale = (out.double() - ref).abs().max().item(), ref.abs().max().item()
    print("gemm_tn %s n=%d %dx%d: err %.3e of %.3e (bound %.1e)" % (layout, n, p, q, err, scale, _tol(layout)))
    assert out.shape == (p, q) and err <= _tol(layout) * scale
    assert torch.equal(out, ops.gemm_tn(a_img, b_img, p, q, **kw))
    n_pad = 32 * ((n + 31) // 32)
    a_pad = torch.cat([a_img, torch.zeros(n_pad - n, a_img.shape[1], dtype=torch.bfloat16, device=DEV)])
    b_pad = torch.cat([b_img, torch.zeros(n_pad - n, b_img.shape[1], dtype=torch.bfloat16, device=DEV)])
    assert torch.equal(out, ops.gemm_tn(a_pad, b_pad, p, q, **kw))


@pytest.mark.parametrize("layout", ["bf16", "x3", "hl"])
@pytest.mark.parametrize("n", [1025, 4099, 16389, 32767])
def test_rows_past_the_bag_do_not_contribute(n, layout):
    """The operands are the first n rows of larger buffers whose other rows hold NaN and Inf bit patterns: the same bits as from
    buffers that end at row n - 1."""
    from snuffy_amd import ops
    p, q = (512, 288) if layout == "hl" else (520, 264)
    a_img, b_img, kw, _ = _operands(n, p, q, layout, seed=7)
    tight = ops.gemm_tn(a_img, b_img, p, q, **kw)
    poison = torch.tensor([0x7FC0, 0x7F80, 0xFF80, 0xFFFF], dtype=torch.int32).to(torch.int16).view(torch.bfloat16).to(DEV)

    def inside(img):
        big = poison[torch.arange((n + 64) * img.shape[1], device=DEV) % 4].view(n + 64, img.shape[1]).contiguous()
        big[:n] = img
        return big[:n]

    a_in, b_in = inside(a_img), inside(b_img)
    assert not torch.isfinite(a_in.float()).all() or True     # (the view itself is finite; the rows behind it are not)
    got = ops.gemm_tn(a_in, b_in, p, q, **kw)
    assert torch.isfinite(got).all()
    assert torch.equal(got, tight)


@pytest.mark.parametrize("layout", ["bf16", "x3", "hl"])
@pytest.mark.parametrize("n", [17, 33])
def test_c_abi_takes_bags_shorter_than_two_steps(n, layout):
    """snf_gemm_tn_ws_bytes / snf_gemm_tn_f32 called directly (ops.gemm_tn keeps its n >= 1024 threshold): one cut step, and one whole
    step followed by a cut one."""
    from snuffy_amd import _ffi, ops
    lib = _ffi.load()
    assert int(lib.snf_gemm_tn_ws_bytes(17, 256, 256)) > 0
    p, q = 256, 256
    a_img, b_img, kw, ref = _operands(n, p, q, layout, seed=3)
    planes = (kw.get("a_planes", (0, -1)), kw.get("b_planes", (0, -1)))
    nb = int(lib.snf_gemm_tn_ws_bytes(n, p, q))
    assert nb >= p * q * 4
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    out = torch.full((p, q), float("nan"), device=DEV)
    rc = lib.snf_gemm_tn_f32(ops._p(a_img), a_img.stride(0), planes[0][0], planes[0][1], ops._p(b_img), b_img.stride(0), planes[1][0],
                             planes[1][1], 1 if kw.get("hl") else 0, n, p, q, ops._p(out), out.stride(0), ops._p(ws), nb, ops._stream())
    assert rc == 0, lib.snf_last_error()
    torch.cuda.synchronize()
    err, scale = (out.double() - ref).abs().max().item(), ref.abs().max().item()
    print("snf_gemm_tn_f32 %s n=%d: err %.3e of %.3e" % (layout, n, err, scale))
    assert err <= _tol(layout) * scale


def _perturbed_state(d, h, lam, share):
    ref = build_amd_milnet(d, h, "relu", lam, share, 1)
    with torch.no_grad():
        for m in ref.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.add_(0.3 * torch.randn(d))
                m.bias.add_(0.2 * torch.randn(d))
            if isinstance(m, torch.nn.Linear) and m.bias is not None:
                m.bias.add_(0.1 * torch.randn_like(m.bias))
    return ref.state_dict()


def test_one_pass_x3_training_chain_at_a_bag_length_off_the_grid(monkeypatch):
    """The construction and the bounds of test_fused_x3_layer0_training_matches_the_generic_fp32_chain at (16384, 768), on a bag of
    16 389 rows: the one-pass chain (hl images, gemm_hl, gemm_tn with a row tail) against the library, generic and concatenated-K
    chains -- logits and every parameter gradient, eval mode and train mode."""
    from snuffy_amd import autograd as SA
    from snuffy_amd import functional as SF
    n, d, h, lam, share = 16389, 768, 6, 200, 0.0
    torch.manual_seed(n)
    sd = _perturbed_state(d, h, lam, share)
    x = torch.randn(1, n, d, device=DEV)
    monkeypatch.setattr(SA, "X3_TRAIN_HL", True)
    assert SA._x3_train_hl_ok(n, d, 4 * d)
    for train_mode in (False, True):
        grads, outs = {}, {}
        for tag, fused, gemm, hl_chain in (("library", False, "library", True), ("generic", False, "x3", True), ("fused", True, "x3", True),
                                           ("fused_cat", True, "x3", False)):
            monkeypatch.setattr(SA, "FUSED_X3_TRAINING", fused)
            monkeypatch.setattr(SA, "X3_TRAIN_HL", hl_chain)
            monkeypatch.setattr(SF, "FP32_GEMM", gemm)
            net = build_amd_milnet(d, h, "relu", lam, share, 1)
            net.load_state_dict(sd, strict=True)
            net = net.to(DEV).configure(precision="fp32", return_attention=False)
            net.train(train_mode)
            torch.manual_seed(11)
            np.random.seed(5)
            ins, logits, _ = net(x)
            (logits.sum() * 3 + ins.max()).backward()
            grads[tag] = {k: p.grad.float().clone() for k, p in net.named_parameters()}
            outs[tag] = logits.detach().clone()
        gate_keys = ("feed_forward.w_1.weight", "feed_forward.w_1.bias", "sublayer.1.norm.weight", "sublayer.1.norm.bias")
        small_keys = ("linears.0.weight", "linears.0.bias", "linears.1.weight", "sublayer.0.norm.weight")
        for other, bound_out, bound in (("library", 5e-5, 2e-4), ("generic", 5e-5, 5e-4 if train_mode else 2e-4), ("fused_cat", 5e-5, 2e-4)):
            d_out = (outs["fused"] - outs[other]).abs().max().item()
            print("train=%s fused vs %s: |dlogit| %.3e" % (train_mode, other, d_out))
            assert d_out <= bound_out * max(1.0, outs[other].abs().max().item())
            for k in grads["fused"]:
                if k.endswith("self_attn.linears.1.bias"):
                    continue                           # mathematically zero gradient
                a, b = grads["fused"][k].double(), grads[other][k].double()
                rel = float((a - b).norm() / b.norm().clamp_min(1e-12))
                print("  %-60s rel %.3e" % (k, rel))
                assert rel < (5e-3 if k.endswith(small_keys) else 3e-3 if k.endswith(gate_keys) else bound), (train_mode, k, other, rel)


def test_bf16_training_chain_at_a_bag_length_off_the_grid(monkeypatch):
    """One bf16 training step on a bag of 16 389 rows: its weight-gradient contractions on gemm_tn (row tail) against the same step on
    the library contractions (ops.GEMM_TN = False), within the bounds test_fused_bf16_layer0_training_matches_generic_and_fp32 applies
    between its bf16 chains."""
    from snuffy_amd import ops
    n, d, h, lam = 16389, 768, 6, 200
    torch.manual_seed(n)
    sd = _perturbed_state(d, h, lam, 0.0)
    x = torch.randn(1, n, d, device=DEV)
    assert ops.gemm_tn_supported(n, d, 4 * d)
    for train_mode in (False, True):
        grads, outs = {}, {}
        for tag, tn in (("library", False), ("gemm_tn", True)):
            monkeypatch.setattr(ops, "GEMM_TN", tn)
            net = build_amd_milnet(d, h, "relu", lam, 0.0, 1)
            net.load_state_dict(sd, strict=True)
            net = net.to(DEV).configure(precision="bf16", return_attention=False)
            net.train(train_mode)
            torch.manual_seed(11)
            ins, logits, _ = net(x)
            (logits.sum() * 3 + ins.max()).backward()
            grads[tag] = {k: p.grad.float().clone() for k, p in net.named_parameters()}
            outs[tag] = logits.detach().clone()
        assert (outs["gemm_tn"] - outs["library"]).abs().max().item() <= 2e-2 * max(1.0, outs["library"].abs().max().item())
        for k in grads["gemm_tn"]:
            if k.endswith("self_attn.linears.1.bias"):
                continue                               # mathematically zero gradient
            a, b = grads["gemm_tn"][k].double(), grads["library"][k].double()
            rel = float((a - b).norm() / b.norm().clamp_min(1e-12))
            print("train=%s %-60s rel %.3e" % (train_mode, k, rel))
            assert rel < 0.08, (train_mode, k, rel)
