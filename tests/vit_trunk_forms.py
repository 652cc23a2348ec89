"""What the suites of the frozen-trunk training route (ssl_pretrain.FUSED_TRUNK) and tools/vit_trunk_train_time.py share: the shape
tables, the operands, the float64 references and the gates, with the reasoning behind each gate."""
import copy
import functools
import math

import torch

DEV = "cuda:0"

# (m, n, view): the row kernels of csrc/vit_train.hip.  One item (4 columns of one row), a row count off the workgroup's 256 items,
# several workgroups, the widest hidden layer of the recipes (4 x 384) over more than one grid-stride trip of a narrow row, and a
# row-strided operand (a column slice of a wider tensor).
KERNEL_SHAPES = [(1, 32, False), (33, 64, False), (111, 256, False), (257, 1536, False), (65, 256, True)]
PLANTED = [0.0, -0.0, 1e-30, -1e-30, 6.0, -6.0, 40.0, -40.0]

# The split keeps 16 significant bits of a value (hi = bf16(v) keeps 8, lo = bf16(v - hi) the next 8): 2^-17 relative at worst, 2^-16 with
# the fp32 rounding of the value before the split.  One more bit is allowed for the fp32 erff / expf: the cap is 2^-15 of the largest
# element, and no gate below is looser.  The gates themselves are 4 x the largest value measured over KERNEL_SHAPES in both formats
# (profiles/vit_trunk_train.txt), one digit up.
KERNEL_CAP = 2.0 ** -15
GELU_GATE = 7e-6                 # 4 x 1.53e-6
GELU_BWD_GATE = 2e-5             # 4 x 4.47e-6
assert GELU_GATE <= KERNEL_CAP and GELU_BWD_GATE <= KERNEL_CAP

# (B, T, D, h, bottleneck) of one frozen block, switch on against off.  m = 34 is off every tile grid and takes the cat form; the hl
# case is BLOCK_HL with B found at run time (hl_batch).
BLOCK_SHAPES = [(2, 17, 64, 1, 8), (3, 37, 128, 2, 8)]
BLOCK_HL = (197, 256, 4, 8)      # T, D, h, bottleneck
ONOFF_GATE = 2e-4                # the fp32-class on / off bound of the attention rows (tests/vit_attn_forms.py): a cap


def rel_err(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def kernel_operands(m, n, strided, seed=0):
    """pre and da [m, n] f32 on the device: normal draws scaled by 3 with PLANTED at the front of row 0 (pre) and of the last row (da)."""
    g = torch.Generator().manual_seed(100 * m + n + seed)
    lo = 64 if strided else 0
    wide = [3.0 * torch.randn(m, n + 2 * lo, generator=g) for _ in range(2)]
    wide[0][0, lo:lo + len(PLANTED)] = torch.tensor(PLANTED)
    wide[1][-1, lo:lo + len(PLANTED)] = torch.tensor(PLANTED)
    pre, da = (w.to(DEV)[:, lo:lo + n] for w in wide)
    assert pre.is_contiguous() is not strided
    return pre, da


def decode(img, fmt, n):
    """(hi, lo) [m, n] bf16 of an image; for cat also asserts that its two hi planes agree."""
    m = img.shape[0]
    if fmt == "hl":
        v = img.view(m, n // 32, 2, 32)
        return v[:, :, 0].reshape(m, n), v[:, :, 1].reshape(m, n)
    assert torch.equal(img[:, :n].view(torch.int16), img[:, n:2 * n].view(torch.int16))
    return img[:, :n], img[:, 2 * n:]


def gelu64(x):
    x = x.double()
    return 0.5 * x * (1.0 + torch.erf(x * math.sqrt(0.5)))


def gelu_slope64(x):
    x = x.double()
    return 0.5 * (1.0 + torch.erf(x * math.sqrt(0.5))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def kernel_errors(ops, m, n, strided):
    """{(kernel, fmt): max |a - b| / max |b| of the decoded image against float64 of the same fp32 operands}."""
    pre, da = kernel_operands(m, n, strided)
    out = {}
    for fmt in ("hl", "cat"):
        hi, lo = decode(ops.gelu_image(pre, fmt), fmt, n)
        out[("gelu", fmt)] = rel_err(hi.double() + lo.double(), gelu64(pre))
        hi, lo = decode(ops.gelu_bwd_image(da, pre, fmt), fmt, n)
        out[("gelu_bwd", fmt)] = rel_err(hi.double() + lo.double(), da.double() * gelu_slope64(pre))
    return out


def small_model(img=32, embed=64, heads=1, depth=3, bott=8, seed=3):
    """A ViT with adapters of `depth` blocks, nothing at its init value, adapter dropout 0, on the CPU in train mode."""
    from snuffy_amd import vit
    from tests.helpers import vit_block_state
    model = vit.VisionTransformer(img_size=[img], patch_size=16, embed_dim=embed, depth=depth, num_heads=heads, mlp_ratio=4, qkv_bias=True,
                                  norm_layer=functools.partial(torch.nn.LayerNorm, eps=1e-6), adapter_ffn_layernorm_option="none",
                                  adapter_ffn_init_option="lora", adapter_ffn_scalar="0.1", adapter_ffn_num=bott, adapter_d_model=embed)
    missing = model.load_state_dict(vit_block_state(embed, depth, bott, seed=seed), strict=False)
    assert not [k for k in missing.missing_keys if k.startswith("blocks.")] and not missing.unexpected_keys
    for m in model.modules():
        if isinstance(getattr(m, "dropout", None), float):
            m.dropout = 0.0
    return model.train()


def freeze_trunk(module):
    for n, p in module.named_parameters():
        p.requires_grad = "adaptmlp" in n
    return module


def frozen_block(d, h, bott, seed=0):
    return freeze_trunk(small_model(embed=d, heads=h, depth=1, bott=bott, seed=seed).blocks[0]).to(DEV)


def block_operands(b, t, d):
    g = torch.Generator().manual_seed(5)
    return torch.randn(b, t, d, generator=g).to(DEV), torch.randn(b, t, d, generator=g).to(DEV)


def run_block(S, blk, x0, dy):
    """[(name, tensor)]: y, dx and the adapter's four gradients of one block_autograd step."""
    blk.zero_grad(set_to_none=True)
    x = x0.clone().requires_grad_(True)
    y = S.block_autograd(blk, x, True)
    y.backward(dy.to(y.dtype))
    return [("y", y.detach()), ("dx", x.grad)] + [(n, p.grad.clone()) for n, p in blk.adaptmlp.named_parameters() if p.grad is not None and p.numel() > 1]


def block_float64(S, blk, x0, dy):
    """The same step of a float64 copy of the block (the torch composition: the route and the attention kernels serve no float64)."""
    return run_block(S, copy.deepcopy(blk).double(), x0.double(), dy.double())


def hl_batch(ops, t, d):
    """The smallest B for which the fc1 projection of B * t rows fills the chip with the one-pass kernel's tiles."""
    b = 1
    while not ops.hl_eligible(b * t, 4 * d, d):
        b += 1
        assert b < 4096
    return b


def count_gemms(monkeypatch, ops):
    """Recorders on ops.gemm_hl and ops.gemm_x3 -> the list of (name, m, n) they append to."""
    calls = []
    for name in ("gemm_hl", "gemm_x3"):
        real = getattr(ops, name)

        def wrapped(a, w, *args, _real=real, _name=name, **kw):
            calls.append((_name, a.shape[0], w.shape[0]))
            return _real(a, w, *args, **kw)

        monkeypatch.setattr(ops, name, wrapped)
    return calls
