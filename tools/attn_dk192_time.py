"""What the dk = 192 kernels of the bf16 MFMA sparse attention (the reference README's MAE recipe: D = 768, h = 4, Lambda = 500 as 250 top
+ 250 random) gain over the routes that head width took before, in THIS tree and -- interleaved, same box, same session -- in another
checkout of the project (--other, e.g. the parent commit built next to this one).

    python tools/attn_dk192_time.py [--other PATH] [--series 4] [--steps 16] [--reps 20] [--out FILE]

(a) the attention alone at (N, K, h, dk) = (30 000, 500, 4, 192), bf16 Q | V as the halves of one [N, 2D] buffer, rotating over three
    operand sets: forward -- ops.sparse_attn_fwd_mfma where the tree has the dk = 192 kernels, and in every tree the route of before: fp32
    copies of Q and V into the exact kernel ops.sparse_attn_fwd (the copies are timed with it: they are part of that route); backward,
    attention dropout 0.1 -- ops.sparse_attn_bwd_mfma from the forward's lse and the Philox state where the tree takes it, and in every
    tree the generic chain's route: ops.sparse_attn_bwd with the fp32 P and a mask tensor.
(b) the model: the bf16 eval forward of the MAE recipe at N = 30 000 and its bf16 training step (BagParallelStepper, attention dropout 0.1,
    encoder dropout 0 and 0.1), in this tree with the switches functional.MFMA_ATTN_DK192 / autograd.FUSED_BF16_DK192 on and off; and the
    config-B eval forward and training step (D = 768, h = 6, Lambda = 200) as the no-regression control.

A series is one child process under `timeout`; the trees alternate series by series (this, other, this, ...), timing is by HIP events
after a warm-up and a pre-roll, the first child that fails ends the run."""
import argparse
import os
import subprocess
import sys
import time

N = 30000
ATTN = (4, 192, 500)
# name, D, h, Lambda, random_patch_share
MODELS = (("MAE_D768_h4_L500_r0.5", 768, 4, 500, 0.5), ("cfgB_D768_h6_L200", 768, 6, 200, 0.0))
STATE = (0.1, 2 ** 63 + 12345, 2 ** 61 + 77)


def _time(fn, reps):
    """ms per call: fn(i) is called with a running index (the caller rotates its operands over it)."""
    import torch
    for i in range(3):
        fn(i)
    torch.cuda.synchronize()
    t0, i = time.perf_counter(), 0
    while time.perf_counter() - t0 < 0.3:                # pre-roll: clocks up, the library's algorithms chosen
        fn(i)
        i += 1
        torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def attn_leg(root, reps):
    sys.path.insert(0, root)
    import torch
    from snuffy_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    h, dk, k = ATTN
    d = h * dk
    tag = "N%d_K%d_h%d_dk%d" % (N, k, h, dk)
    new = hasattr(ops, "mfma_attn_dk192_supported") and ops.mfma_attn_dk192_supported(k, N, 2 * d)
    sets = []
    for _ in range(3):                                   # rotating operands: 3 x 92 MB of Q | V, more than the last-level cache
        qv = torch.randn(N, 2 * d, generator=g).to(dev).to(torch.bfloat16)
        sets.append((qv[:, :d], qv[:, d:], torch.randn(k, d, generator=g).to(dev), torch.randn(k, d, generator=g).to(dev)))
    ms = _time(lambda i: ops.sparse_attn_fwd(sets[i % 3][0].float(), sets[i % 3][2], sets[i % 3][1].float(), h), reps)
    print("RESULT what=attn_fwd:%s:fp32_copies+exact chain=- ms=%.4f" % (tag, ms), flush=True)
    if new:
        kp16 = [s[2].to(torch.bfloat16) for s in sets]
        ms = _time(lambda i: ops.sparse_attn_fwd_mfma(sets[i % 3][0], sets[i % 3][1], kp16[i % 3], N, h), reps)
        print("RESULT what=attn_fwd:%s:mfma chain=- ms=%.4f" % (tag, ms), flush=True)
    # backward: the generic chain's route (fp32 operands, P [h, N, K] from the forward, the mask as a tensor) on ONE operand set -- P and
    # the mask are 240 MB each, far beyond any cache, so the set need not rotate
    q, v, kp, dout = sets[0]
    qf, vf = q.float(), v.float()
    _, p, _ = ops.sparse_attn_fwd(qf, kp, vf, h, need_attn=True)
    mask = ops.dropout_mask(h, N, k, STATE[0], STATE[1], STATE[2], dev)
    ms = _time(lambda i: ops.sparse_attn_bwd(qf, kp, vf, p, dout, h, mask=mask), reps)
    print("RESULT what=attn_bwd:%s:exact_P+mask chain=- ms=%.4f" % (tag, ms), flush=True)
    del p, mask, qf, vf
    if new:
        lses = [ops.sparse_attn_fwd_mfma(s[0], s[1], s[2], N, h, need_lse=True)[2] for s in sets]
        ms = _time(lambda i: ops.sparse_attn_bwd_mfma(sets[i % 3][0], sets[i % 3][1], sets[i % 3][2], sets[i % 3][3], lses[i % 3], h,
                                                      dropout=STATE, fused_bf16_grads=True), reps)
        print("RESULT what=attn_bwd:%s:mfma_chunked chain=- ms=%.4f" % (tag, ms), flush=True)


def model_leg(root, steps):
    sys.path.insert(0, root)
    import torch
    import bench
    from snuffy_amd import autograd as SA
    from snuffy_amd import functional as SF
    from snuffy_amd.train import BagParallelStepper
    dev = torch.device("cuda:0")
    new = hasattr(SA, "FUSED_BF16_DK192")
    g = torch.Generator().manual_seed(1)
    bags = [torch.randn(1, N, 768, generator=g).to(dev) for _ in range(3)]
    lab = [torch.tensor([float(i % 2)], device=dev) for i in range(3)]
    for name, D, heads, lam, share in MODELS:
        for switch in ((True, False) if (new and name.startswith("MAE")) else (None,)):
            if switch is not None:
                SF.MFMA_ATTN_DK192 = switch
                SA.FUSED_BF16_DK192 = switch
            sw = "-" if switch is None else ("on" if switch else "off")
            net = bench.build_net(D, heads, lam, "bf16", dev, share).eval()
            calls = []
            real_fwd = SF.ops.sparse_attn_fwd_mfma
            SF.ops.sparse_attn_fwd_mfma = lambda *a, **kw: (calls.append(1), real_fwd(*a, **kw))[1]

            def fwd(i):
                with torch.no_grad():
                    net(bags[i % 3])
            fwd(0)
            SF.ops.sparse_attn_fwd_mfma = real_fwd
            ms = _time(fwd, steps)
            print("RESULT what=eval:%s:switch_%s chain=%s ms=%.4f" % (name, sw, "mfma" if calls else "exact", ms), flush=True)
            del net
            for p in (0.0, 0.1):
                net = bench.build_net(D, heads, lam, "bf16", dev, share)
                layer = net.b_classifier.encoder.layers[0]
                for drop in (layer.sublayer[0].dropout, layer.sublayer[1].dropout, layer.feed_forward.dropout):
                    drop.p = p                               # what --encoder_dropout sets; attention dropout stays at its 0.1
                st = BagParallelStepper(net, world_size=1, dist=None, device=dev, precision="bf16")
                calls = []
                real = SA.EncoderLayer0Bf16Fn.apply
                SA.EncoderLayer0Bf16Fn.apply = lambda *a: (calls.append(1), real(*a))[1]
                st.step(bags[0], lab[0])
                torch.cuda.synchronize()
                chain = "fused" if calls else "generic"
                SA.EncoderLayer0Bf16Fn.apply = real
                ms = _time(lambda i: st.step(bags[i % 3], lab[i % 3]), steps)
                print("RESULT what=step:%s:enc_p%.1f:switch_%s chain=%s ms=%.4f" % (name, p, sw, chain, ms), flush=True)
                del st, net


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", help="root of another checkout (built) to time against, series interleaved with this tree's")
    ap.add_argument("--series", type=int, default=4)
    ap.add_argument("--steps", type=int, default=16, help="calls per figure of the model forwards and steps")
    ap.add_argument("--reps", type=int, default=20, help="launches per figure of the attention alone")
    ap.add_argument("--only", choices=("attn", "model"), help="one of the two parts")
    ap.add_argument("--out")
    ap.add_argument("--leg", metavar="ROOT", help="one series of the tree at ROOT, in this process (what the driver starts)")
    ap.add_argument("--part", choices=("attn", "model"))
    args = ap.parse_args()
    if args.leg:
        attn_leg(args.leg, args.reps) if args.part == "attn" else model_leg(args.leg, args.steps)
        return 0
    trees = [("this", here)] + ([("other", os.path.abspath(args.other))] if args.other else [])
    res, chains, lines = {}, {}, []

    def say(s):
        lines.append(s + "\n")
        print(s, flush=True)

    def flush():
        if args.out:
            open(args.out, "w").writelines(lines)

    for part in ("attn", "model"):
        if args.only and args.only != part:
            continue
        for s in range(args.series):
            for tag, root in trees:
                cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--leg", root, "--part", part,
                       "--steps", str(args.steps), "--reps", str(args.reps)]
                r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, cwd=root)
                if r.returncode != 0:
                    say("series %d (%s) of tree %s ended with status %d: stopping" % (s, part, tag, r.returncode))
                    flush()
                    return r.returncode
                for line in r.stdout.splitlines():
                    if line.startswith("RESULT"):
                        f = dict(kv.split("=", 1) for kv in line.split()[1:])
                        res.setdefault((tag, f["what"]), []).append(float(f["ms"]))
                        chains[(tag, f["what"])] = f["chain"]
                        say("series %d  %-5s %s" % (s, tag, line[7:]))
            flush()
    say("")
    say("N = %d, bf16, attention dropout 0.1 in training; %d series, ms per call / per step (fastest and median series per figure)"
        % (N, args.series))
    for (tag, what), ms in sorted(res.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        srt = sorted(ms)
        med = srt[len(srt) // 2] if len(srt) % 2 else 0.5 * (srt[len(srt) // 2 - 1] + srt[len(srt) // 2])
        say("%-5s %-52s [%-7s]  %s   min %.4f  median %.4f  max %.4f  spread %.2f %%" % (
            tag, what, chains[(tag, what)], "  ".join("%.4f" % v for v in ms), srt[0], med, srt[-1], 100 * (srt[-1] - srt[0]) / srt[0]))
    flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
