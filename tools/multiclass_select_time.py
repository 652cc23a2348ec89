"""What the one-launch class-union selector and the batched layer route buy the multiclass model (snuffy_multiclass.FUSED_SELECT,
snuffy_multiclass.PACK_BATCH), against the parent's paths in the same process.

    python tools/multiclass_select_time.py [--iters 30] [--out profiles/multiclass_select.txt]

Table 1: EncoderLayer.select at (B, N, C, Lambda), random_patch_share 0.5 -- select_unfused (per-class launches, torch.unique and a device ->
host copy per row, numpy draws), the fused form with numpy's draws (sampler "reference") and with the device sampler.
Table 2: the whole eval forward of MILNet (critic, one encoder layer, head; C = 2, Lambda = 200, random_patch_share 0.5, return_attention
off) with PACK_BATCH off (the row loop) and on, fp32-class and bf16.
Every figure is the median over --iters calls of a HIP-event pair around one call (the stream is idle when the first event is recorded, so
host-side gaps inside the call count), after a warm-up of the same call; every configuration is run twice to show the run-to-run spread."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SELECT_SHAPES = [(1, 10000, 2, 200), (1, 32768, 2, 200), (8, 4000, 2, 200), (1, 70000, 2, 200)]
FORWARD_SHAPES = [(8, 4000, 512, 8), (4, 16000, 512, 4)]
R = 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    from snuffy_amd import snuffy_multiclass as smc
    if not torch.cuda.is_available():
        print("no GPU: nothing measured")
        return 1
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        lines.append(s + "\n")
        print(s, flush=True)
        if args.out:
            open(args.out, "w").writelines(lines)

    def median_ms(fn):
        for _ in range(args.warmup):
            fn()
        ts = []
        for _ in range(args.iters):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts))

    def build(D, h, lam, C=2):
        torch.manual_seed(0)
        layer = smc.EncoderLayer(D, smc.MultiHeadedAttention(h, D), smc.PositionwiseFeedForward(D, 4 * D, "relu"), C, 0.0, lam, R)
        net = smc.MILNet(smc.FCLayer(D, C), smc.BClassifier(smc.Encoder(layer, 1), C, D))
        for p in net.parameters():
            if p.dim() > 1:
                torch.nn.init.xavier_normal_(p)
        return net.to(dev).eval()

    say("%s; medians of %d calls after %d warm-up calls, two runs per configuration" % (torch.cuda.get_device_name(0), args.iters, args.warmup))
    say("")
    say("EncoderLayer.select, ms per call (run 1 / run 2); random_patch_share %.1f" % R)
    say("%-22s %6s %19s %19s %19s %9s %9s" % ("(B, N, C, Lambda)", "K", "select_unfused", "fused, reference", "fused, device", "ref x", "device x"))
    for (B, N, C, lam) in SELECT_SHAPES:
        net = build(64, 2, lam, C)
        layer = net.b_classifier.encoder.layers[0]
        c = torch.randn(B, N, C, generator=torch.Generator().manual_seed(N)).to(dev)
        res = {}
        for name in ("unfused", "reference", "device"):
            net.configure(sampler="device" if name == "device" else "reference")
            fn = (lambda: layer.select_unfused(c)) if name == "unfused" else (lambda: layer.select(c))
            res[name] = []
            for _ in range(2):
                np.random.seed(5)
                res[name].append(median_ms(fn))
        k = 2 * layer.select(c)[0].shape[1]
        fmt = lambda v: "%8.3f / %8.3f" % tuple(v)
        say("%-22s %6d %19s %19s %19s %8.2fx %8.2fx" % ((B, N, C, lam), k, fmt(res["unfused"]), fmt(res["reference"]), fmt(res["device"]),
                                                        min(res["unfused"]) / max(res["reference"]), min(res["unfused"]) / max(res["device"])))
    say("(x: slowest run of the fused form against the fastest run of select_unfused)")
    say("")
    say("MILNet eval forward, ms per batch (run 1 / run 2); C = 2, Lambda = 200, one encoder layer, return_attention off, sampler reference")
    say("%-26s %-5s %6s %21s %21s %9s" % ("B x N, D, h", "prec", "K", "row loop", "batched", "speedup"))
    verdict = []
    for (B, N, D, h) in FORWARD_SHAPES:
        net = build(D, h, 200)
        x = torch.randn(B, N, D, generator=torch.Generator().manual_seed(3)).to(dev)
        for precision in ("fp32", "bf16"):
            net.configure(precision=precision, return_attention=False, sampler="reference")

            def fwd():
                with torch.no_grad():
                    net(x)

            res = {False: [], True: []}
            for _ in range(2):
                for on in (False, True):
                    smc.PACK_BATCH = on
                    np.random.seed(5)
                    res[on].append(median_ms(fwd))
            k = 2 * net.b_classifier.encoder.layers[0].last_selection[0].shape[1]
            worst = min(res[False]) / max(res[True])
            verdict.append(worst)
            say("%-26s %-5s %6d %9.3f / %9.3f %9.3f / %9.3f %8.2fx" % ("%d x %d, %d, %d" % (B, N, D, h), precision, k, res[False][0], res[False][1],
                                                                   res[True][0], res[True][1], worst))
        del net, x
    say("(speedup: slowest batched run against the fastest row-loop run)")
    say("PACK_BATCH: batched at least level with the row loop outside the spread at every composition: %s"
        % ("yes" if min(verdict) >= 1.0 else "NO"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
