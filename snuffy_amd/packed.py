"""Many bags per launch: the packed ("varlen") inference forward behind ``MILNet.forward_bags`` /
``forward_packed``.  The reference has no counterpart -- it runs one bag per forward (train.py:468-473 batch_size 1, snuffy.py:130-131
indexes with a 1-D tensor); this is the same per-bag arithmetic over rows packed into one tensor (DESIGN.md section 4 "Varlen path").
Functions take the MILNet as their first argument; ``snuffy.MILNet`` exposes them as methods."""
import math

import numpy as np
import torch

from . import functional as SF
from . import snuffy

# Uniform groups above one key chunk (Lambda > 224 / 256) and at head widths between the kernels' (64 < dk < 128, zero-padded to 128:
# functional.packed_head_pad) -- the README recipes D = 384, h = 4, Lambda = 900 / 500.  False: such bags take the per-bag loop, the
# routing of before.  On: in profiles/varlen_key_chunks.txt (tools/varlen_key_chunks_time.py) the packed route is at least level with the
# loop at every measured composition of both recipes -- 64 x 1000 patches 4.3 - 8.5x, 64 x 8000 1.00 - 1.34x fp32-class / 1.9 - 2.5x bf16,
# the synthetic CAMELYON16-shaped mix 1.1 - 1.95x -- with no crossover in bag length up to PACK_MAX_ROWS per launch set: no length gate.
PACK_KEY_CHUNKS = True
# The random patch share of a packed batch drawn on the device when the model is configured with sampler="device": ONE launch
# (ops.DeviceSampler.draw_packed) for every bag and layer instead of a device -> host copy of the top rows and one np.random.choice per bag
# and layer, several groups (uniform chunks and a ragged group) instead of one, and graph replay under graph_max_patches.  False: the
# routing of before -- host draws whatever the sampler, one uniform group, never captured.  The rule PACK_KEY_CHUNKS follows decides the
# shipped value: on only where the device route is at least level with the host draws at every composition of
# profiles/packed_device_sampler.txt (tools/packed_sampler_time.py).
PACK_DEVICE_SAMPLER = True
# Uniform groups of the bf16 model at head width 192 (the README's MAE recipe: D = 768, h = 4, Lambda = 500 as 250 + 250) on the varlen
# forms of the dk = 192 kernels (ops.varlen_attn_dk192_supported: up to 8 chunks of 128 keys).  False: such bags take the per-bag loop
# (or the ragged kernel where it takes them), the routing of before, call for call.  The rule of PACK_KEY_CHUNKS decides the shipped
# value: on only where the packed route is at least level with the loop at every row of profiles/varlen_dk192.txt
# (tools/varlen_dk192_time.py).  On: 64 x 1000 patches 7.2 - 9.7x, 64 x 8000 2.07 - 2.57x, the synthetic CAMELYON16-shaped mix
# 1.84 - 2.26x, host draws and device sampler, return_attention off and on -- no row behind the loop, so no length gate in dk192_ok.
PACK_DK192 = True
# Uniform groups of the fp32 model at head width 192 on the varlen forms of the fused fp32-class kernel of that width
# (ops.varlen_attn_x3_dk192_supported: up to 8 chunks of 128 keys).  False: such bags take the per-bag loop (or the ragged kernel where it
# takes them), the routing of before, call for call.  Ships off; the rule of PACK_KEY_CHUNKS decides a later flip: on only where the
# packed route is at least level with the loop at every row of profiles/x3_dk192.txt (tools/x3_dk192_time.py).  Independent of
# functional.X3_ATTN_DK192, which routes the single bag.
PACK_X3_DK192 = False
# The same at head width 256 (the README's SimCLR ResNet-18 recipe: D = 512, h = 2, Lambda = 900; ops.varlen_attn_x3_dk256_supported: up
# to 8 chunks of 128 keys).  False: such bags take the per-bag loop (or the ragged kernel where it takes them), the routing of before,
# call for call.  The rule of PACK_KEY_CHUNKS decides the value: on only where the packed route is at least level with the loop at every
# row of profiles/x3_dk256.txt (tools/x3_dk256_time.py).  On: 64 x 1000 patches 4.87 - 5.27x, 64 x 8000 1.18 - 1.26x, the synthetic
# CAMELYON16-shaped mix 1.14 - 1.23x, host draws and device sampler, return_attention off and on -- no row behind the loop, so no length
# gate in x3_dk256_ok.  Independent of functional.X3_ATTN_DK256, which routes the single bag (and stays off).
PACK_X3_DK256 = True
# Uniform groups of the bf16 model at head width 256 (the same recipe in precision="bf16", one encoder layer) on the varlen forms of the
# bf16 kernel of that width (ops.varlen_attn_dk256_supported: up to 8 chunks of 128 keys).  False: such bags take the per-bag loop (or the
# ragged kernel where it takes them), the routing of before, call for call.  The rule of PACK_KEY_CHUNKS decides the value: on only where
# the packed route is at least level with the loop at every row of profiles/attn_dk256.txt (tools/attn_dk256_time.py).  On: 64 x 1000
# patches 5.80 - 6.74x, 64 x 8000 1.58 - 1.78x, the synthetic CAMELYON16-shaped mix 1.51 - 1.71x, host draws and device sampler,
# return_attention off and on -- no row behind the loop, so no length gate in dk256_ok.  Independent of functional.MFMA_ATTN_DK256, which
# routes the single bag (and stays off), and of PACK_X3_DK256 (fp32).
PACK_DK256 = True
RAGGED_MAX_ROWS = 4096      # longest bag the ragged (exact fp32, one workgroup per bag and head) attention is meant for


def pack_groups(net, bags):
    """How forward_bags() packs `bags`: a list of (bag indices, ragged flag) groups, or None (nothing can be packed).

    The packed path covers inference of the binary model with a plain one-logit FCLayer critic.  "uniform" groups (ragged =
    False): every bag has at least Lambda patches, so all select the same K rows, and the head width is one the MFMA kernels
    take -- varlen forms of the bf16 / fp32-class attention kernels (with PACK_KEY_CHUNKS also Lambda above one key chunk and head widths
    between the kernels', zero-padded; with PACK_DK192 also the bf16 model at head width 192, up to 8 chunks of 128 keys -- fp32 at that
    width packs behind PACK_X3_DK192, fp32 at head width 256 behind PACK_X3_DK256, bf16 at that width behind PACK_DK256, and stays per bag without it).  "ragged" groups: bags shorter than Lambda (they select
    ALL their rows, snuffy.py:129) or head widths outside the MFMA kernels (the MIL benchmark sets: D = 166 / 230, h = 2) --
    exact-fp32 ragged attention, bags of at most _RAGGED_MAX_ROWS patches.  With a random share the draws of the reference
    sampler must stay in bag order, so only one uniform group over all bags is formed.  With the device sampler
    (device_draws()) a random-share model is grouped like a deterministic one: uniform groups hold the bags with at least
    k1 + k2 rows, a ragged bag selects its min(k1, n_b) top rows and min(k2, n_b - min(k1, n_b)) random ones, min(k1 + k2, n_b)
    keys.  Philox offsets follow the order in which forward_bags() runs things: the groups in the order returned here (the
    uniform chunks, then the ragged ones), each taking one offset per bag in the group's bag order, then the bags left to the
    per-bag loop in their own order."""
    cfg = net.b_classifier.cfg
    layers = list(net.b_classifier.encoder.layers)
    if (len(bags) < 2 or net.training or torch.is_grad_enabled() or type(net.i_classifier) is not snuffy.FCLayer or not layers
            or not all(type(l) is snuffy.EncoderLayer for l in layers) or cfg.precision not in ("fp32", "bf16")):
        return None
    if net.i_classifier.fc[0].weight.shape[0] != 1:
        return None
    x0 = bags[0]
    for x in bags:
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.device == x0.device
                and ((x.dim() == 3 and x.shape[0] == 1) or x.dim() == 2) and x.shape[-1] == x0.shape[-1]
                and x.shape[-2] >= 1):
            return None
    d = x0.shape[-1]
    h = layers[0].self_attn.h
    if d % h:
        return None
    kb = None
    for l in layers:
        k1 = math.ceil(l.big_lambda * l.top_big_lambda_share)
        k2 = int(l.big_lambda * l.random_patch_share)
        if k1 < 1 or (kb is not None and (k1, k2) != kb) or l.self_attn.h != h:
            return None
        kb = (k1, k2)
    k1, k2 = kb
    if cfg.compute == "bf16" and any(l.sublayer[0].norm.eps != l.sublayer[1].norm.eps for l in layers):
        return None
    sizes = [x.shape[-2] for x in bags]
    uniform_dims = (d % 4 == 0 and (SF.ops.varlen_attn_supported(cfg.compute, k1 + k2, d // h)
                                    or key_chunks_ok(layers, cfg.compute, d, h, k1 + k2, len(bags), sum(sizes))
                                    or any(_wide_ok(row, cfg.compute, d, h, k1 + k2) for row in _WIDE))
                    and (cfg.compute == "bf16" or SF.FP32_ATTENTION == "x3"))
    on_device = k2 > 0 and device_draws(cfg) and SF.ops.draw_packed_supported(min(max(sizes), 65536), k1, k2, len(layers))
    if k2 > 0 and not on_device:
        ok = (uniform_dims and min(sizes) >= k1 + k2 and max(sizes) <= 65536 and (k1 + k2) * len(bags) <= (1 << 20)
              and sum(sizes) <= getattr(net, "_PACK_MAX_ROWS", PACK_MAX_ROWS))      # one group only: the draws must stay in bag order
        return [(list(range(len(bags))), False)] if ok else None
    uni = [i for i, n in enumerate(sizes) if uniform_dims and k1 + k2 <= n <= 65536]
    rest = [i for i in range(len(bags)) if i not in set(uni)]
    rag = [i for i in rest if sizes[i] <= getattr(net, "_RAGGED_MAX_ROWS", RAGGED_MAX_ROWS)]
    if rag and not SF.ops.ragged_attn_supported(min(k1 + k2, max(sizes[i] for i in rag)), d // h):
        rag = []
    groups = []
    for g, r in ((uni, False), (rag, True)):
        groups += [(c, r) for c in chunk_rows(net, g, sizes) if len(c) >= 2]
    return groups or None


def device_draws(cfg):
    """The packed path draws the random share with the device sampler (PACK_DEVICE_SAMPLER and configure(sampler="device"))."""
    return PACK_DEVICE_SAMPLER and cfg.sampler == "device"


# The packed switches of the native head widths: (switch, the precision the model computes in, head width).  Each precision has a
# switch of its own at each width: the bf16 switches leave precision="fp32" per bag and the other way round.
_WIDE = (("PACK_DK192", "bf16", 192), ("PACK_X3_DK192", "fp32", 192), ("PACK_DK256", "bf16", 256), ("PACK_X3_DK256", "fp32", 256))


def _wide_ok(row, compute, d, h, k):
    """A native head width packs: its switch is on, the model computes in the kernel's precision, and the key count is inside the
    varlen kernel of the width's record in ops.SPARSE_ATTN_FORMS."""
    switch, precision, dk = row
    return bool(globals()[switch] and compute == precision and h >= 1 and d == dk * h
                and SF.ops.sparse_attn_form_serves(SF.ops.sparse_attn_form(precision, dk), k))


def dk192_ok(compute, d, h, k):
    """PACK_DK192: the bf16 model at head width 192."""
    return _wide_ok(_WIDE[0], compute, d, h, k)


def x3_dk192_ok(compute, d, h, k):
    """PACK_X3_DK192: the fp32 model at head width 192 (the fused fp32-class varlen kernel of that width)."""
    return _wide_ok(_WIDE[1], compute, d, h, k)


def dk256_ok(compute, d, h, k):
    """PACK_DK256: the bf16 model at head width 256."""
    return _wide_ok(_WIDE[2], compute, d, h, k)


def x3_dk256_ok(compute, d, h, k):
    """PACK_X3_DK256: the fp32 model at head width 256 (the fused fp32-class varlen kernel of that width)."""
    return _wide_ok(_WIDE[3], compute, d, h, k)


def key_chunks_ok(layers, compute, d, h, k, bags, rows):
    """PACK_KEY_CHUNKS: the packed width (functional.packed_head_pad) and the key count are inside the key-chunked varlen kernels, and
    the padded projections' shapes pass the checks the single-bag path applies to them (functional.encoder_layer)."""
    ops = SF.ops
    dk = d // h
    dkp = SF.packed_head_pad(dk)
    if not PACK_KEY_CHUNKS or dkp is None or not ops.varlen_attn_chunks_supported(compute, k, dkp):
        return False
    if dkp == dk:
        return True
    rows = min(rows, PACK_MAX_ROWS)
    kr = min(k * bags, 8192)                                             # _rows_linear_padded slices the B x K selected rows
    if (d % 16 or any(l.self_attn.linears[1].weight.dtype != torch.float32 for l in layers)
            or not ops.linear_rows_x3_supported(kr, h * dkp, d) or not ops.linear_rows_x3_supported(kr, d, h * dkp)):
        return False
    if compute == "bf16":
        return ops.gemm_supported(rows, 2 * h * dkp, d)
    f = layers[0].feed_forward.w_2.weight.shape[1]
    return (SF.FP32_GEMM == "x3" and ops.gemm_supported(rows, d, 3 * f) and ops.gemm_supported(rows, 2 * d, 3 * d)
            and ops.gemm_supported(rows, 2 * h * dkp, 3 * d))


PACK_MAX_ROWS = 196608      # rows of one packed launch set: the GEMMs address their [T, 3F] images with 32-bit element offsets
PACKED_GRAPHS = 32          # captured batch compositions kept per model (oldest dropped first)


def chunk_rows(net, idx, sizes):
    """Split a group into consecutive chunks of at most _PACK_MAX_ROWS packed rows."""
    chunks, cur, rows = [], [], 0
    for i in idx:
        if cur and rows + sizes[i] > getattr(net, "_PACK_MAX_ROWS", PACK_MAX_ROWS):
            chunks.append(cur)
            cur, rows = [], 0
        cur.append(i)
        rows += sizes[i]
    if cur:
        chunks.append(cur)
    return chunks


def packable(net, bags):
    """True when forward_bags() runs ALL of `bags` as one uniform packed batch."""
    groups = pack_groups(net, list(bags))
    return bool(groups) and len(groups) == 1 and not groups[0][1] and len(groups[0][0]) == len(bags)


def forward_bags(net, bags):
    """``[net(x) for x in bags]`` with the bags' rows packed into ONE set of launches (bags of <= 8 k patches
    are launch-latency bound -- ~25 launches per bag whatever its size).  bags: sequence of [1, N_b, D] (or [N_b, D]) fp32 GPU
    tensors.  Returns the list of (classes [1, N_b, 1], prediction_bag [1, C], A [1, h, N_b, K_b] or None) tuples the per-bag
    forwards return: same selections (bit-exact, random share included: the reference sampler's numpy draws are made bag by bag
    in the order the per-bag forwards make them; the device sampler (configure(sampler="device"), PACK_DEVICE_SAMPLER) draws all
    bags and layers of a group in one launch, bag b from the Philox offset the b-th per-bag forward would use -- bit-exact
    against the loop when one uniform group covers all bags in order (packable()), otherwise in the order pack_groups()
    documents -- with no host read, numpy's stream untouched, and graph replay under graph_max_patches).  At kernel level (top-k, attention, head) a bag's result does not depend on what it is packed
    with, bit for bit; the projections pick their kernel by the PACKED row count, so a bag's logits move by fp32 / bf16 rounding
    with the batch composition (metrics computed from packed evaluation carry that rounding).  Against the per-bag forwards the
    top-k and head kernels are bit-identical, the attention sums its partial tiles in another order, and the projections
    run over the packed rows (a library / tile choice that depends on the row count): logits move by fp32 / bf16 rounding.
    Bags that select different numbers of rows (shorter than Lambda) or whose head width the MFMA kernels do not take are
    packed as a second, "ragged" group (pack_groups); head width 192 (D = 768, h = 4) packs in bf16 behind PACK_DK192 and
    in fp32 behind PACK_X3_DK192 (off: per bag), head width 256 (D = 512, h = 2) in fp32 behind PACK_X3_DK256 and in bf16 behind PACK_DK256; whatever cannot be packed (training, multiclass critic, ...) takes
    the per-bag loop."""
    bags = list(bags)
    groups = pack_groups(net, bags)
    if not groups:
        return [net(x) for x in bags]
    out = [None] * len(bags)
    lim = getattr(net, "_graph_max_patches", 0)
    graph_ok = lim > 0 and (all(l.random_patch_share == 0 for l in net.b_classifier.encoder.layers)
                            or device_draws(net.b_classifier.cfg))      # a selection that stays on the device
    for idx, ragged in groups:
        sizes = tuple(bags[i].shape[-2] for i in idx)
        rows = [bags[i].reshape(-1, bags[i].shape[-1]) for i in idx]
        if graph_ok and max(sizes) <= lim:
            res = forward_bags_graph(net, rows, sizes, ragged)
        else:
            packed = packed_cache(net, sizes, rows[0].device)
            res = split_packed(forward_packed_raw(net, torch.cat(rows), packed, ragged), packed)
        for i, r in zip(idx, res):
            out[i] = r
    for i, x in enumerate(bags):
        if out[i] is None:
            out[i] = net(x)
    return out


def packed_cache(net, sizes, device):
    """PackedBags (offsets + launch plans) of the most recent batch compositions."""
    cache = net.__dict__.setdefault("_packed_bags", {})
    key = (sizes, str(device))
    pk = cache.get(key)
    if pk is None:
        if len(cache) >= 64:
            cache.pop(next(iter(cache)))
        pk = cache[key] = SF.ops.PackedBags(sizes, device)
    return pk


def forward_bags_graph(net, rows, sizes, ragged=False):
    """forward_bags() as ONE captured HIP graph per batch composition (configure(graph_max_patches=...), deterministic
    selection or the device sampler's random share): the bags are copied into the graph's static packed buffer and the ~30
    launches replay without the host.  The device sampler's record is advanced inside the graph, so every replay draws fresh
    rows; a graph is bound to the record it was captured with (and keeps it alive)."""
    sig = net._weights_signature()
    if sig != getattr(net, "_graph_sig", None):
        net._graphs.clear()
        net._graph_seen.clear()
        net._graph_sig = sig
    cfg = net.b_classifier.cfg
    dev = rows[0].device
    key = ("bags", sizes, bool(ragged), dev, cfg.precision, cfg.return_attention)
    sampler = None
    if device_draws(cfg) and any(l.random_patch_share > 0 for l in net.b_classifier.encoder.layers):
        sampler = cfg.device_sampler(dev)
        key += (sampler.state.data_ptr(),)
    ent = net._graphs.get(key)
    if ent is None:
        packed = packed_cache(net, sizes, dev)
        if key not in net._graph_seen:
            # a composition is captured only when it comes back (a capture costs three extra forwards and pins a [T, D] buffer):
            # a loader that never repeats a batch stays on the eager path
            if len(net._graph_seen) > 8192:
                net._graph_seen.clear()
            net._graph_seen.add(key)
            return split_packed(forward_packed_raw(net, torch.cat(rows), packed, ragged), packed)
        static_x = torch.cat(rows)
        try:
            cur = torch.cuda.current_stream()
            side = getattr(net, "_capture_stream", None)
            if side is None or side.device != dev:
                side = net._capture_stream = torch.cuda.Stream(dev)      # warm-up AND capture run on this stream
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                sel_state = SF.ops.fresh_selector(dev)                   # this graph's own selector state
                for _ in range(2):
                    forward_packed_raw(net, static_x, packed, ragged)
            cur.wait_stream(side)
            if net._graph_pool is None:
                net._graph_pool = torch.cuda.graph_pool_handle()
            graph = torch.cuda.CUDAGraph()
            graph._snf_selector = sel_state
            graph._snf_sampler = sampler                   # the record's address is baked into the capture
            with torch.cuda.graph(graph, pool=net._graph_pool, stream=side, capture_error_mode="thread_local"):
                out = forward_packed_raw(net, static_x, packed, ragged)
        except Exception as exc:
            import warnings
            warnings.warn("snuffy_amd: HIP-graph capture of the packed inference forward failed (%s: %s); graph replay is "
                          "disabled for this model" % (type(exc).__name__, exc), RuntimeWarning, stacklevel=2)
            net._graph_max_patches = 0
            torch.cuda.synchronize()
            return split_packed(forward_packed_raw(net, torch.cat(rows), packed, ragged), packed)
        if len(net._graphs) >= net._GRAPH_SHAPES:
            net._graphs.pop(next(iter(net._graphs)))
        held = [k for k in net._graphs if k and k[0] == "bags"]
        if len(held) >= PACKED_GRAPHS:                 # every packed graph pins its own packed input buffer
            net._graphs.pop(held[0])
        ent = net._graphs[key] = (graph, static_x, out, packed)
    graph, static_x, out, packed = ent
    torch.cat(rows, out=static_x)
    graph.replay()
    # the graphs share one pool: outputs are valid until the next replay -- three copies per batch, then per-bag views
    return split_packed(tuple(o.clone() if isinstance(o, torch.Tensor) else o for o in out), packed)


def forward_packed(net, x_cat, packed, ragged=False):
    """forward_bags() on rows that are already packed: x_cat [T, D] fp32, packed = ops.PackedBags(sizes, device) (keep it
    between calls with the same bag sizes: it caches the launch plans).  ragged: the bags select different numbers of rows
    (some are shorter than Lambda) or the head width is outside the MFMA kernels -- deterministic selection, or a random share drawn
    by the device sampler (device_draws())."""
    return split_packed(forward_packed_raw(net, x_cat, packed, ragged), packed)


def split_packed(raw, packed):
    s, logits, attn, kbs = raw
    out = []
    for b, n in enumerate(packed.sizes):
        lo = int(packed.host[b])
        a_b = None
        if attn is not None:
            a_b = attn[:, :, lo:lo + n, :] if kbs is None else attn[:, :, lo:lo + n, :kbs[b]]
        out.append((s[lo:lo + n].view(1, n, -1), logits[b].view(1, -1), a_b))
    return out


def forward_packed_raw(net, x_cat, packed, ragged=False):
    """(critic scores [T, 1], logits [B, C], A [1, h, T, K] or None, per-bag key counts or None) over the packed rows."""
    enc = net.b_classifier.encoder
    cfg = net.b_classifier.cfg
    layers = list(enc.layers)
    lin = net.i_classifier.fc[0]
    x_cat = SF.as_2d(x_cat)
    for layer in layers[:1]:
        layer._xhat_offer = None
        layer._xn3_offer = None
    if cfg.compute == "bf16":
        eps = layers[0].sublayer[0].norm.eps
        s, xhat = SF.ops.critic_ln(x_cat, lin.weight, lin.bias, eps)            # same kernel as the per-bag critic pass
        layers[0]._xhat_offer = (x_cat.data_ptr(), tuple(x_cat.shape), x_cat._version, float(eps), xhat)
    else:
        # fp32-class: where the layer takes the one-pass GEMMs, the critic pass also leaves LayerNorm_0's image (one read of the rows)
        s = SF.critic_scores_with_hl(x_cat, lin.weight, lin.bias, layers[0])
    c1 = s.reshape(-1)
    l0 = layers[0]
    k1 = math.ceil(l0.big_lambda * l0.top_big_lambda_share)
    k2 = int(l0.big_lambda * l0.random_patch_share)
    top = SF.ops.topk_segmented(c1, packed, k1)                                   # [B, k1] inside each bag
    first = packed.dev[:-1].unsqueeze(1)
    rnd = rag = None
    on_device = k2 > 0 and device_draws(cfg) and SF.ops.draw_packed_supported(packed.max_n, k1, k2, len(layers))
    if on_device:
        if not ragged and min(packed.sizes) < k1 + k2:
            raise SF.SnuffyHipError("a uniform packed group needs at least Lambda = %d rows per bag (shortest: %d): pass ragged=True"
                                    % (k1 + k2, min(packed.sizes)))
        # every bag's and every layer's draw in one launch, bag b from the offset the b-th per-bag forward would use; no host read
        rnd = cfg.device_sampler(top.device).draw_packed(packed, k1, k2, top, len(layers))      # [layers, B, k2]
    if ragged:
        if k2 > 0 and not on_device:
            raise SF.SnuffyHipError("ragged packed bags support the deterministic selection (random_patch_share == 0) or the device "
                                    "sampler (configure(sampler='device')) only")
        # a bag shorter than Lambda selects all of its rows (snuffy.py:129): per-bag key counts, selected rows concatenated
        rag = packed.ragged([min(k1 + k2, n) for n in packed.sizes])
        pos, base = rag.flat_index(k1) if k2 == 0 else ragged_random_index(packed, rag, k1, k2)
        sel_ragged = top.reshape(-1)[pos] + base if k2 == 0 else None
    elif k2 > 0 and not on_device:
        # the reference's draws (snuffy.py:134-143), in the order the per-bag forwards consume the global numpy stream:
        # bag by bag, and inside a bag layer by layer (every layer draws from the complement of the same `top`)
        top_h = top.cpu().numpy()
        draws = np.empty((len(layers), packed.bags, k2), dtype=np.int64)
        for b, n in enumerate(packed.sizes):
            mask = np.ones(n, dtype=bool)
            mask[top_h[b]] = False
            remaining = np.nonzero(mask)[0]
            for li in range(len(layers)):
                draws[li, b] = np.random.choice(remaining, k2, replace=False)
        rnd = torch.from_numpy(draws).to(top.device)                             # [layers, B, k2]
    parts = attn = None
    x2 = x_cat
    for li, layer in enumerate(layers):
        if parts is not None:
            x2 = SF.materialize(parts)
        layer.last_selection = None
        layer.last_selection_bags = (top, None if rnd is None else rnd[li])     # ragged: entries >= K_b of a row are padding
        if ragged and k2 > 0:      # bag b: top[b, :min(k1, n_b)] ++ rnd[li, b, :k2_b], the valid entries of the padded [B, k1 + k2] rows
            sel = torch.cat((top, rnd[li]), dim=1).reshape(-1)[pos] + base
        elif ragged:
            sel = sel_ragged
        else:
            sel_local = top if rnd is None else torch.cat((top, rnd[li]), dim=1)  # [B, K]: top ++ random, as snuffy.py:145
            sel = (sel_local + first).reshape(-1)
        parts, attn = SF.encoder_layer(x2, sel, layer, (li == len(layers) - 1) and cfg.return_attention, cfg.compute,
                                       packed=packed, ragged=rag)
    logits = SF.head(parts, enc.norm, net.b_classifier.linear, packed=packed)   # [B, C]
    return s, logits, attn, (rag.kbs if rag is not None else None)



def ragged_random_index(packed, rag, k1, k2):
    """RaggedKeys.flat_index for rows laid out as top [B, k1] ++ random [B, k2]: the positions of bag b's min(k1, n_b) top rows and of its
    min(k2, n_b - min(k1, n_b)) random rows in the flattened [B, k1 + k2] array, and the bag's first packed row per entry (device int64,
    built from the bag sizes alone and cached on the PackedBags)."""
    key = ("ragged_random", k1, k2)
    hit = packed._plans.get(key)
    if hit is None:
        pos = []
        for b, n in enumerate(packed.sizes):
            t = min(k1, n)
            r = min(k2, n - t)
            pos.append(b * (k1 + k2) + np.arange(t, dtype=np.int64))
            pos.append(b * (k1 + k2) + k1 + np.arange(r, dtype=np.int64))
        base = np.repeat(packed.host[:-1], rag.kbs)
        hit = packed._plans[key] = (torch.from_numpy(np.concatenate(pos)).to(packed.device), torch.from_numpy(base).to(packed.device))
    return hit
