"""MI355X-native drop-in for the reference's ``snuffy_multiclass.py`` (batched / multi-class Snuffy).

Same module API as the reference (snuffy_multiclass.py:60-253): ``EncoderLayer(size, self_attn, feed_forward, num_class,
dropout, big_lambda, random_patch_share)`` with ``forward(x, c, current_layer)``, ``BClassifier`` with ``feats_size`` /
``num_class`` attributes, batches B >= 1, C >= 1 classes.  Everything that is shape-identical to the binary model is
re-used from ``snuffy_amd.snuffy`` (same state-dict keys); only the selection differs (snuffy_multiclass.py:130-171):

  per batch row: top ceil(Lambda(1-r)) indices PER CLASS (descending score), flattened row-major over (rank, class),
  torch.unique (ascending); ref_dim = min over rows of the unique count, then min(ref_dim, N - ref_dim); keep the LOWEST
  ref_dim unique indices; draw ref_dim random indices from the complement of ALL uniques of that row (np.random.choice
  on the global numpy RNG, row after row); K = 2 * ref_dim.

The selection is ONE launch for the whole batch (ops.multiclass_select: per-class exact top-k and the ascending union, one workgroup
per row) and one device -> host copy, which the tensor shape K = 2 * ref_dim makes unavoidable; the random rows are numpy's (default,
the reference's stream bit for bit) or the device sampler's (RuntimeConfig.set_sampler("device"): no further host traffic).  The layer
math runs on the same fused kernels as the binary model: an inference batch of B >= 2 rows as ONE packed launch set (the varlen kernels
of packed.py, B bags of equal length), everything else one bag row at a time.  Training goes through the same autograd functions as the
binary model (every parameter gradient checked against autograd through the CPU oracle, tests/test_gpu_train.py).
"""
import math

import numpy as np
import torch
import torch.nn as nn

from . import functional as SF
from . import ops
from .snuffy import (FCLayer, IClassifier, MILNet, MultiHeadedAttention, PositionwiseFeedForward,  # noqa: F401
                     RuntimeConfig, SublayerConnection, _share_config, attention, clones)

device = torch.device("cuda" if torch.cuda.is_available() else "cpu")

# One-launch class-union selection (csrc/topk.hip: multiclass_select_kernel).  False: the per-class launches + torch.unique of before
# (EncoderLayer.select_unfused).  On: the selections and numpy's stream position are bit-identical by test, and the fused form issues
# one launch and one device -> host copy where the other issues C launches, a unique and a copy per batch row.
FUSED_SELECT = True
# Inference batches of B >= 2 rows as one packed launch set (_pack_batch_ok).  False: the row loop of before.  Timings of both routes:
# profiles/multiclass_select.txt (tools/multiclass_select_time.py); the switch is on only if the packed forward is at least level with the
# loop at every measured composition, outside the run-to-run spread -- the rule of packed.PACK_KEY_CHUNKS.
PACK_BATCH = True
_PACKED_BAGS = {}


class EncoderLayer(nn.Module):
    "Per-class top-Lambda + equal-size random set, sparse attention on the selected rows, feed forward."

    def __init__(self, size, self_attn, feed_forward, num_class, dropout, big_lambda, random_patch_share):
        super(EncoderLayer, self).__init__()
        self.self_attn = self_attn
        self.feed_forward = feed_forward
        self.sublayer = clones(SublayerConnection(size, dropout), 2)
        self.size = size
        self.big_lambda = big_lambda
        self.random_patch_share = random_patch_share
        self.top_big_lambda_share = 1.0 - random_patch_share
        self.num_classes = num_class
        self.last_selection = None
        self.cfg = RuntimeConfig()
        _share_config(self, self.cfg)

    def select_unfused(self, c):
        """select() as it was before the one-launch selector: per class an ops.topk on a strided column, torch.unique per row, the
        numpy draws behind a device -> host copy per row.  Always the reference's host draws."""
        b, n, ncls = c.shape
        k1 = min(math.ceil(self.big_lambda * self.top_big_lambda_share), n)
        uniq = []
        for i in range(b):
            cols = [ops.topk(c[i, :, cc], k1) for cc in range(ncls)]            # exact selector on a strided column
            flat = torch.stack(cols, dim=1).reshape(-1)                           # (rank, class) row-major = reference
            uniq.append(torch.unique(flat))                                       # ascending
        ref_dim = min(int(u.numel()) for u in uniq)
        ref_dim = min(ref_dim, n - ref_dim)
        topk = torch.stack([u[:ref_dim] for u in uniq]) if ref_dim > 0 else \
            torch.zeros(b, 0, dtype=torch.int64, device=c.device)
        rnd = torch.zeros(b, ref_dim, dtype=torch.int64)
        for i in range(b):
            mask = np.ones(n, dtype=bool)
            mask[uniq[i].cpu().numpy()] = False                                   # device->host, as .tolist() in the reference
            remaining = np.nonzero(mask)[0]
            rnd[i] = torch.from_numpy(np.random.choice(remaining, ref_dim, replace=False).astype(np.int64))
        return topk, rnd.to(c.device)

    def select(self, c, layer_index=0):
        """c [B, N, C] on the GPU -> (topk [B, ref_dim] int64, rnd [B, ref_dim] int64) as the reference builds them."""
        b, n, ncls = c.shape
        k1 = min(math.ceil(self.big_lambda * self.top_big_lambda_share), n)
        if not (FUSED_SELECT and ops.multiclass_select_supported(b, n, ncls, k1)):
            return self.select_unfused(c)
        uniq, counts = ops.multiclass_select(c, k1)                               # [B, C k1] ascending unions, [B] their lengths
        # ONE device -> host copy: K = 2 ref_dim is a tensor shape, so the counts must be read
        host = torch.cat((counts.to(torch.int64).unsqueeze(1), uniq), dim=1).cpu().numpy()
        cnt = host[:, 0]
        ref_dim = int(cnt.min())
        ref_dim = min(ref_dim, n - ref_dim)
        if ref_dim <= 0:
            empty = torch.zeros(b, 0, dtype=torch.int64, device=c.device)
            return empty, empty.clone()
        topk = uniq[:, :ref_dim]                                                  # the LOWEST ref_dim unique indices of every row
        if ref_dim > n - int(cnt.max()):
            raise ValueError("Cannot take a larger sample than population when 'replace=False'")   # numpy's own refusal
        if self.cfg.sampler == "device" and b <= 64 and layer_index < 64:        # no further host traffic
            return topk, self.cfg.device_sampler(c.device).draw_batch(n, ref_dim, uniq, counts, layer=layer_index)
        rnd = np.empty((b, ref_dim), dtype=np.int64)
        for i in range(b):                                                        # the reference's draws, row after row
            mask = np.ones(n, dtype=bool)
            mask[host[i, 1:1 + cnt[i]]] = False
            remaining = np.nonzero(mask)[0]
            rnd[i] = np.random.choice(remaining, ref_dim, replace=False)
        return topk, torch.from_numpy(rnd).to(c.device)                           # one host -> device copy of all rows

    def run(self, x, c, need_attn=True, layer_index=0):
        """x [B, N, D] -> (list of Parts per row, A [B, h, N, K] or None); on the batched route (_pack_batch_ok) ONE Parts over the
        packed [B N, D] rows instead of the list."""
        topk, rnd = self.select(c, layer_index)
        self.last_selection = (topk, rnd)
        sel = torch.cat((topk, rnd), dim=1)
        if _pack_batch_ok(self, self.cfg, x, sel.shape[1]):
            b, n, d = x.shape
            packed = _packed_bags(b, n, x.device)
            flat = (sel + packed.dev[:-1].unsqueeze(1)).reshape(-1)               # packed coordinates: bag b's K rows at [b K, (b + 1) K)
            parts, attn = SF.encoder_layer(x.reshape(b * n, d), flat, self, need_attn, self.cfg.compute, packed=packed)
            if attn is not None:                                                  # [1, h, B N, K] -> [B, h, N, K], a view
                attn = attn.view(attn.shape[1], b, n, attn.shape[3]).transpose(0, 1)
            return parts, attn
        parts, attns = [], []
        for i in range(x.shape[0]):
            p, a = SF.encoder_layer(x[i].contiguous(), sel[i].contiguous(), self, need_attn, self.cfg.compute)
            parts.append(p)
            attns.append(a)
        attn = torch.cat(attns, dim=0) if need_attn else None
        return parts, attn

    def forward(self, x, c, current_layer):
        xb = _as_batch(x)
        if self.cfg.sampler == "device":
            self.cfg.device_sampler(xb.device).advance()     # a layer called on its own (not through Encoder.run_layers): fresh rows per call
        parts, attn = self.run(xb, c, self.cfg.return_attention)
        return _rows(parts, xb.shape[0]), attn


def _rows(parts, b):
    "z [B, N, D] of one layer's result: per-row Parts, or Parts over the packed rows of the batched route."
    if isinstance(parts, list):
        return torch.stack([SF.materialize(p) for p in parts])
    z = SF.materialize(parts)
    return z.view(b, -1, z.shape[1])


def _packed_bags(b, n, dev):
    "PackedBags of B bags of N rows (offsets + launch plans), cached per (B, N, device)."
    key = (b, n, str(dev))
    pk = _PACKED_BAGS.get(key)
    if pk is None:
        if len(_PACKED_BAGS) >= 64:
            _PACKED_BAGS.pop(next(iter(_PACKED_BAGS)))
        pk = _PACKED_BAGS[key] = ops.PackedBags([n] * b, dev)
    return pk


def _pack_batch_ok(layer, cfg, x, k):
    """The batched route of one layer: inference, B >= 2, K >= 1 keys per row, and shapes the packed kernels take -- the predicates
    packed.pack_groups applies to a uniform group."""
    from . import packed as PK
    if not PACK_BATCH or torch.is_grad_enabled() or x.dim() != 3 or x.shape[0] < 2 or k < 1:
        return False
    b, n, d = x.shape
    h = layer.self_attn.h
    if d % h or d % 4 or b * n > PK.PACK_MAX_ROWS or n > 65536 or k > n:
        return False
    compute = cfg.compute
    if compute not in ("fp32", "bf16") or (compute == "fp32" and SF.FP32_ATTENTION != "x3"):
        return False
    if compute == "bf16" and layer.sublayer[0].norm.eps != layer.sublayer[1].norm.eps:
        return False
    return bool(ops.varlen_attn_supported(compute, k, d // h) or PK.key_chunks_ok([layer], compute, d, h, k, b, b * n))


def _as_batch(x):
    if x.dim() != 3:
        raise ValueError("expected [B, N, D], got %s" % (tuple(x.shape),))
    if not x.is_cuda:
        from ._ffi import SnuffyHipError
        raise SnuffyHipError("input must be a GPU tensor: snuffy_amd has no CPU fallback")
    return x.float().contiguous()


class Encoder(nn.Module):
    "Stack of N layers followed by LayerNorm.  Reference snuffy_multiclass.py:75-89."

    def __init__(self, layer, N):
        super(Encoder, self).__init__()
        self.layers = clones(layer, N)
        self.norm = nn.LayerNorm(layer.size)
        self.cfg = RuntimeConfig().bind_stack(self.layers)
        _share_config(self, self.cfg)

    def run_layers(self, x, c):
        """x [B, N, D] -> (Parts of the last layer: a list per row, or ONE over the packed rows on the batched route; A)."""
        parts, attn = None, None
        n_layers = len(self.layers)
        if self.cfg.sampler == "device":
            self.cfg.device_sampler(x.device).advance()      # a fresh Philox offset per forward, as snuffy.Encoder
        b = x.shape[0]
        for li, layer in enumerate(self.layers):
            if parts is not None:
                x = _rows(parts, b)
            parts, attn = layer.run(x, c, need_attn=(li == n_layers - 1) and self.cfg.return_attention, layer_index=li)
        return parts, attn

    def forward(self, x, c):
        xb = _as_batch(x)
        parts, attn = self.run_layers(xb, c)
        if isinstance(parts, list):
            z = torch.stack([SF.layer_norm(SF.materialize(p), self.norm) for p in parts])
        else:
            z = SF.layer_norm(SF.materialize(parts), self.norm).view(xb.shape[0], xb.shape[1], -1)
        return z, attn


class BClassifier(nn.Module):
    "Reference snuffy_multiclass.py:60-72."

    def __init__(self, encoder, num_classes, input_size: int):
        super(BClassifier, self).__init__()
        self.encoder = encoder
        self.linear = nn.Linear(input_size, num_classes)
        self.feats_size = input_size
        self.num_class = num_classes
        self.cfg = RuntimeConfig().bind_stack(getattr(encoder, "layers", None))
        _share_config(self, self.cfg)

    def configure(self, precision=None, return_attention=None):
        self.cfg.set(precision, return_attention)
        return self

    def forward(self, x, c):
        "x [B, N, D], c [B, N, C] -> (logits [B, C], A [B, h, N, K])"
        xb = _as_batch(x)
        parts, attn = self.encoder.run_layers(xb, c.float())
        if isinstance(parts, list):
            logits = torch.stack([SF.head(p, self.encoder.norm, self.linear) for p in parts])
        else:                                                # batched route: one head launch over the packed rows -> [B, C]
            logits = SF.head(parts, self.encoder.norm, self.linear, packed=_packed_bags(xb.shape[0], xb.shape[1], xb.device))
        return logits, attn
