"""The register forms of the row passes (csrc/rowops.hip: critic_kernel, layernorm_rows_kernel, ln_bwd_rows_kernel, ln_colsum_kernel), as
the tests see them: the widths that reach every (VEC, NV) form at both of its edges, the row counts that walk the grid-stride loop one,
two and three times, the entries that launch each kernel, and the operands, fp64 references and image decoders the form tests share.
Plain data and small helpers, no test functions: test_row_forms_host.py proves the table complete (every entry x every form it admits,
no device needed), test_gpu_row_forms.py runs it.

Tolerances are the ones the project already gates each kernel with (the literals below name the test they come from); no row of the
table needed another.  One that does gets 4 x the error of the same formula evaluated in plain fp32 torch against fp64 at its shape,
with the measured value next to it -- never a bound taken from the kernel's output."""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

from tests.helpers import DEV, _ln_reference, _ops, _split_host

EPS = 1e-5

# ---- the forms ---------------------------------------------------------------------------------------------------------------------------
# (vec, nv): a wave holds nv groups of 64 vectors of vec floats, so the form's widest row is 64 * vec * nv
VEC4_FORMS = [(4, nv) for nv in (1, 2, 3, 4, 6, 8)]
VEC1_FORMS = [(1, nv) for nv in (1, 2, 3, 4, 8, 16, 32)]
FORMS = VEC4_FORMS + VEC1_FORMS


def form_rule(d, aligned):
    """The rule of pick_row_cfg, restated: the narrowest form that holds d floats, or None."""
    vec, nvs = (4, (1, 2, 3, 4, 6, 8)) if d % 4 == 0 and aligned else (1, (1, 2, 3, 4, 8, 16, 32))
    return next(((vec, nv) for nv in nvs if 64 * vec * nv >= d), None)


def form_edges(form, hl=False):
    """(bottom, top) widths of a form: one vector past the previous form's top (only lane 0 of the last group is live) and its own top
    (every lane live).  A scalar form's own top is a multiple of 4, which aligned operands take in 16-byte vectors: its top edge by width
    is one short of it (WIDTHS_VEC1_ALIGN reaches the top itself).  hl: the entries that need d % 32 == 0 -- the bottom edge is one
    32-column chunk past the previous top (lanes 0 - 7 of the last group)."""
    vec, nv = form
    forms = VEC4_FORMS if vec == 4 else VEC1_FORMS
    i = forms.index(form)
    below = 64 * vec * forms[i - 1][1] if i else 0
    return below + (32 if hl else vec), 64 * vec * nv - (vec == 1)


# ---- widths ------------------------------------------------------------------------------------------------------------------------------
WIDTHS_VEC4 = [4, 256, 260, 512, 516, 768, 772, 1024, 1028, 1536, 1540, 2048]
WIDTHS_VEC1 = [1, 63, 65, 127, 129, 191, 193, 255, 257, 511, 513, 1023, 1025, 2047]
WIDTHS_VEC1_ALIGN = [256, 768, 2048]      # d % 4 == 0 with every f32 operand 4 bytes off a 16-byte boundary: the scalar fallback
WIDTHS_HL = [32, 256, 288, 512, 544, 768, 800, 1024, 1056, 1536, 1568, 2048]     # the hl image needs d % 32 == 0, so only VEC = 4
TOO_WIDE = [(2052, True), (2049, True)]   # (d, aligned): refused by every entry before any launch
TOO_WIDE_HL = 2080                        # the narrowest refused width that passes the hl entries' d % 32 == 0 check

# (d, aligned) of every case of a kernel that takes any width / of the long row counts (a narrow, a middle and a wide form per VEC)
CASES = [(d, True) for d in WIDTHS_VEC4 + WIDTHS_VEC1] + [(d, False) for d in WIDTHS_VEC1_ALIGN]
LONG_CASES = [(d, True) for d in (260, 768, 2048, 193, 1025)]
LONG_HL = [768, 2048]
DEFERRED_WIDTHS = [768, 1028, 193]        # VEC4 NV3; VEC4 NV6 over five column blocks; VEC1 NV4
VARLEN_WIDTHS = [768, 193]


def case_id(case):
    return "d%d%s" % (case[0], "" if case[1] else "-off4")


# ---- entries: which widths reach which kernel ---------------------------------------------------------------------------------------------
# name -> (kernel, the (d, aligned) cases the form tests launch it at).  The host test requires every form the widths admit.
_HL = [(d, True) for d in WIDTHS_HL]
ENTRIES = {
    "critic": ("critic_kernel", CASES),
    "critic_ln": ("critic_kernel", CASES),
    "critic_ln_hl": ("critic_kernel", _HL),
    "layernorm_rows": ("layernorm_rows_kernel", CASES),
    "layernorm_rows_split3": ("layernorm_rows_kernel", _HL + [(d, True) for d in WIDTHS_VEC1]),
    "layernorm_rows_hl": ("layernorm_rows_kernel", _HL),
    "layernorm_rows_hl_patch_": ("layernorm_rows_kernel", _HL),
    "layernorm_rows_bwd": ("ln_bwd_rows_kernel", CASES),
    "ln_mean_head": ("ln_colsum_kernel", CASES),
}
# critic_select, the deferred head and the varlen head run at the long cases only; their forms are a subset of the entries above
HL_ONLY = ("critic_ln_hl", "layernorm_rows_hl", "layernorm_rows_hl_patch_")


# ---- the library's own figures -------------------------------------------------------------------------------------------------------------
def lib():
    return _ops()._ffi.load()


def row_form(d, aligned):
    """(vec, nv) snf_row_form picks, or None where it refuses the width."""
    vec, nv = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib().snf_row_form(int(d), int(bool(aligned)), ctypes.byref(vec), ctypes.byref(nv))
    if rc:
        assert rc == _ops()._ffi.SNF_EUNSUPPORTED and b"too wide" in lib().snf_last_error(), rc
        return None
    return vec.value, nv.value


def rows_per_trip():
    """Rows one trip of the grid-stride loop of the critic, LayerNorm and backward kernels covers on this device (4 waves a workgroup)."""
    return 4 * lib().snf_layernorm_bwd_blocks(10 ** 9)


def head_rows_per_trip():
    """... and of the head's column-sum kernel: 4 x the workgroups the plan gives a huge bag."""
    off = np.array([0, 10 ** 9], dtype=np.int64)
    need = ctypes.c_size_t(0)
    fn = lib().snf_ln_mean_head_varlen_plan
    assert fn(ctypes.c_void_p(off.ctypes.data), 1, 64, None, 0, ctypes.byref(need), None) == 0
    table = np.zeros(need.value, dtype=np.int32)
    assert fn(ctypes.c_void_p(off.ctypes.data), 1, 64, ctypes.c_void_p(table.ctypes.data), table.size, ctypes.byref(need), None) == 0
    return 4 * int(table[3])


def colsum_long_rows():
    """More than 32 rows per workgroup of colsum_fused and a ragged last workgroup."""
    return 32 * lib().snf_colsum_blocks(10 ** 9) + 33


SHORT_ROWS = [1, 3, 37]                   # one wave; a partly empty workgroup; a few workgroups


def long_rows(per_trip):
    """Two trips, and three with a ragged last one (one full workgroup and one row)."""
    return [per_trip + 5, 2 * per_trip + 4 + 1]


def trips(n, per_trip):
    return -(-n // per_trip)


# ---- tolerances (the project's own) ----------------------------------------------------------------------------------------------------------
LN_F32, LN_BF16, LN_MEAN, LN_RSTD_REL = 2e-5, 2e-2, 1e-5, 1e-5        # test_layernorm_rows, inputs randn * 3 + 1
BWD_DX_REL, BWD_PARAM_REL = 2e-5, 1e-4                                # test_layernorm_rows_bwd_kernel
REF64_FLOOR = 1e-12     # at d = 1 the exact dx is 0 and the bound relative to it with it: the fp64 reference's own rounding, far below fp32's
CRITIC = 2e-5                                                         # test_critic
HEAD = 1e-5                                                           # test_ln_mean_head: pooled, logits, z_out


def colsum_tol(ref, n):
    return 2e-5 * max(1.0, ref.abs().max().item()) * (n ** 0.5)       # test_colsum_fused_kernel


# ---- operands ----------------------------------------------------------------------------------------------------------------------------
def gen(*seed):
    return torch.Generator(device=DEV).manual_seed(sum(int(s) * 7919 ** i for i, s in enumerate(seed)) % (2 ** 31))


def rows_operand(g, n, d, scale, shift):
    """[n, d] on the device: randn * scale + shift, row i also carries 0.01 * (i % 97) -- no two neighbouring rows share a mean."""
    x = torch.randn(n, d, generator=g, device=DEV) * scale + shift
    return x + 0.01 * (torch.arange(n, device=DEV) % 97).float().unsqueeze(1)


def columns(g, *shape, scale=1.0, shift=0.0):
    """gamma / beta / w: random in every column."""
    return torch.randn(*shape, generator=g, device=DEV) * scale + shift


def place(t, aligned):
    """t itself, or its copy one element into a buffer one element longer: a contiguous view 4 bytes off its 16-byte boundary."""
    if aligned or t is None:
        return t
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def slot_of(n, rows, device=DEV):
    """(slot map [n] int32 with rows[j] -> j, rows as a tensor)"""
    rows = torch.as_tensor(sorted(set(int(r) for r in rows)), dtype=torch.int64)
    slot = torch.full((n,), -1, dtype=torch.int32)
    slot[rows] = torch.arange(rows.numel(), dtype=torch.int32)
    return slot.to(device), rows.to(device)


def marked_rows(n, per_trip):
    """Row 0, row n - 1, one inside and, where the loop runs more than once, the first row of the last trip."""
    last_trip = (trips(n, per_trip) - 1) * per_trip
    return sorted({0, n // 2, n - 1, last_trip})


# ---- fp64 references -----------------------------------------------------------------------------------------------------------------------
def ln64(x, gamma=None, beta=None):
    return F.layer_norm(x.double(), (x.shape[1],), None if gamma is None else gamma.double(), None if beta is None else beta.double(), EPS)


def ln_bwd64(x, dy, gamma, residual):
    """(dx, dgamma, dbeta) of LayerNorm by fp64 autograd; dy [n, d] or one broadcast row [d]; gamma None: ones."""
    g = gamma if gamma is not None else torch.ones(x.shape[1], device=x.device)
    return _ln_reference(x, dy.float() if dy.dim() == 2 else dy.float().unsqueeze(0), g, EPS, residual)


def head64(zsum, gamma, beta, w, b):
    """(pooled, logits) = Linear(mean_n LN(z')) in fp64 of the assembled rows z' (fp64)."""
    pooled = F.layer_norm(zsum, (zsum.shape[1],), gamma.double(), beta.double(), EPS).mean(0)
    return pooled, F.linear(pooled, w.double(), None if b is None else b.double())


# ---- images --------------------------------------------------------------------------------------------------------------------------------
def decode_hl(img, d):
    """(hi, lo) [n, d] bf16 of the interleaved image [n, 2 d]: every 32 columns as [hi(32) | lo(32)]."""
    n = img.shape[0]
    v = img.view(n, d // 32, 2, 32)
    return v[:, :, 0].reshape(n, d), v[:, :, 1].reshape(n, d)


def decode_split3(img, d):
    """(hi, hi again, lo) of the [hi | hi | lo] image [n, 3 d]."""
    return img[:, :d], img[:, d:2 * d], img[:, 2 * d:]


def split(x):
    return _split_host(x)


# ---- a synthetic deferred K part ------------------------------------------------------------------------------------------------------------
def deferred_pattern(tm, tn, band_stride):
    """Whether tile (tm, tn) has a slab: differs between neighbouring row bands, neighbouring column blocks and between the bands one
    wave visits on consecutive trips (band_stride row bands apart)."""
    return (tm * 3 + tn + tm // max(band_stride, 1)) % 2 == 1


def synthetic_deferred(g, n, d, rows_per_trip_):
    """ops.DeferredK over O(1) random slabs, one per tile the pattern names, numbered in a shuffled order (a map entry that is stale or
    shifted by one names another slab, or none)."""
    tiles_m, tiles_n = (n + 255) // 256, (d + 255) // 256
    stride = max(rows_per_trip_ // 256, 1)
    cells = [(tm, tn) for tm in range(tiles_m) for tn in range(tiles_n) if deferred_pattern(tm, tn, stride)]
    order = torch.randperm(len(cells), generator=torch.Generator().manual_seed(n + d)).tolist()
    tile_map = torch.zeros(tiles_m, tiles_n, dtype=torch.int32)
    for (tm, tn), s in zip(cells, order):
        tile_map[tm, tn] = s + 1
    slabs = torch.randn(len(cells), 256, 256, generator=g, device=DEV)
    return _ops().DeferredK(slabs, tile_map.to(DEV), None)
