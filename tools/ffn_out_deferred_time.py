"""Development: config B's FFN output projection with the split-K sum inside the GEMM (ops.gemm_hl) against the deferred form
(ops.gemm_hl_deferred), the head on a summed z against the head that adds the deferred part, and the two pairs back to back as the
model issues them; device events over 300 launches, three rounds (profiles/ffn_out_deferred_split.txt)."""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from snuffy_amd import ops

def timeit(fn, n=300):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n

m, n, k = 32768, 768, 3072
a = ops.split_hl_rows(torch.randn(m, k, device="cuda"))
w = ops.split_hl_weight(torch.randn(n, k, device="cuda") / k ** 0.5)
b = torch.randn(n, device="cuda")
res = torch.randn(m, n, device="cuda")
z_split = ops.gemm_hl(a, w, b, resid=res)
z, dk = ops.gemm_hl_deferred(a, w, b, resid=res)
zsum = dk.add_to(z)
print("deferred vs split-K at config B: max |d| = %.3e (scale %.2f), map nonzero %d" % ((zsum - z_split).abs().max().item(), z_split.abs().max().item(), int((dk.tile_map != 0).sum())), flush=True)
d = n
gamma, beta = torch.ones(d, device="cuda"), torch.zeros(d, device="cuda")
wh, bh = torch.randn(1, d, device="cuda"), torch.zeros(1, device="cuda")
sel = torch.randperm(m)[:200]
slot = torch.full((m,), -1, dtype=torch.int32); slot[sel] = torch.arange(200, dtype=torch.int32); slot = slot.cuda()
delta = torch.randn(200, d, device="cuda")
l0 = ops.ln_mean_head(zsum, gamma, beta, 1e-5, wh, bh, slot=slot, delta_rows=delta)
l1 = ops.ln_mean_head(z, gamma, beta, 1e-5, wh, bh, slot=slot, delta_rows=delta, deferred=dk)
print("head on summed z vs deferred: equal logits %s pooled %s" % (torch.equal(l0[0], l1[0]), torch.equal(l0[1], l1[1])), flush=True)
for rnd in range(3):
    t_split = timeit(lambda: ops.gemm_hl(a, w, b, resid=res))
    t_def = timeit(lambda: ops.gemm_hl_deferred(a, w, b, resid=res))
    t_h0 = timeit(lambda: ops.ln_mean_head(zsum, gamma, beta, 1e-5, wh, bh, slot=slot, delta_rows=delta))
    t_h1 = timeit(lambda: ops.ln_mean_head(z, gamma, beta, 1e-5, wh, bh, slot=slot, delta_rows=delta, deferred=dk))
    # producer -> consumer back to back, as the model issues them (the slabs are freshly written when the head reads them)
    def pair_split():
        zz = ops.gemm_hl(a, w, b, resid=res)
        ops.ln_mean_head(zz, gamma, beta, 1e-5, wh, bh, slot=slot, delta_rows=delta)
    def pair_def():
        zz, dd = ops.gemm_hl_deferred(a, w, b, resid=res)
        ops.ln_mean_head(zz, gamma, beta, 1e-5, wh, bh, slot=slot, delta_rows=delta, deferred=dd)
    t_p0, t_p1 = timeit(pair_split), timeit(pair_def)
    print("round %d: FFN-out split-K %.1f us, deferred %.1f us | head (3 launches) plain %.1f us, deferred %.1f us | GEMM + head: %.1f -> %.1f us"
          % (rnd, t_split, t_def, t_h0, t_h1, t_p0, t_p1), flush=True)
