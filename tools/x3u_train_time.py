"""What autograd.X3U_TRAINING buys fp32 training at the head widths outside the pipelined x 3 kernels (dk = 96 / 192 / 256): one optimizer
step of train.BagParallelStepper at precision="fp32", return_attention off, on the three recipes of the reference README that run there.

    python tools/x3u_train_time.py [--rounds 3] [--window 0.5] [--out profiles/x3u_train.txt]

  switch off   the routing of before: exact vector-ALU forward (ops.sparse_attn_fwd), the Philox keep-mask written as an [h, N, K] tensor,
               p * mask and O recomputed by torch.bmm, the exact backward reading the mask tensor
  switch on    the unfused fp32-class pair (ops.sparse_attn_fwd_x3u) with the mask regenerated in its pooling pass, the exact backward
               regenerating it too: no mask tensor, no bmm
Rows: the SimCLR recipe (D 512, h 2, Lambda 900, share 7/9, gelu, depth 5, encoder dropout 0.2: the generic chain, SparseAttnFn in every
layer), the MAE recipe (D 768, h 4, Lambda 500, share 0.5, relu, depth 1, encoder dropout 0) and the DINO-from-scratch recipe (D 384, h 4,
Lambda 900, share 7/9, relu, depth 1, encoder dropout 0.1), both on EncoderLayer0X3Fn; each at N = 8000 and N = 32768, attention dropout 0.1.
First the forward alone at the recipes' attention shapes (device events): the pair without dropout, with it (the difference is what the
Philox rounds of the pooling pass cost next to its MFMAs), and the forward of the routing before with its mask tensor and bmm.

One process; the two routes alternate round by round; every step figure is a host clock around steps that end in a device synchronise, over
a window of --window seconds after a warm-up of the same shape.  The spread is min / median / max of the rounds; a row is BEHIND when the
medians' ratio is under 1 and the ranges do not overlap, LEVEL when they do (the ship rule: on only if no row is behind outside the
run-to-run spread) -- the protocol of tools/attn_dk256_train_time.py."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RECIPES = (("simclr_resnet18", 512, 2, 900, 7 / 9, "gelu", 5, 0.2),
           ("mae_adapter", 768, 4, 500, 0.5, "relu", 1, 0.0),
           ("dino_scratch", 384, 4, 900, 7 / 9, "relu", 1, 0.1))
BAGS = (8000, 32768)


def build_net(dev, d, h, lam, share, act, depth, enc_drop):
    """bench.build_net's initialisation on the recipe's model."""
    import torch
    from snuffy_amd.snuffy import build_milnet
    torch.manual_seed(0)
    net = build_milnet(d, h, act, lam, share, depth, encoder_dropout=enc_drop)
    for _, p in net.named_parameters():
        if p.dim() > 1:
            torch.nn.init.xavier_normal_(p)
    for m in net.modules():
        if isinstance(m, torch.nn.Linear):
            torch.nn.init.zeros_(m.bias)
    return net.to(dev)


def forwards(say, dev, reps=20):
    """The attention forward alone, microseconds by device events (median of `reps` after a warm-up), and the dropped O of the pair against
    the fp64 product of its own P, the mask tensor and V."""
    import torch
    from snuffy_amd import ops
    say("attention forward alone, us (median of %d, device events); O err = the pair's dropped O against fp64 (P o M)^T V (bound 2e-5)" % reps)
    say("%-22s %12s %12s %12s %14s %10s" % ("(n, k, h, dk)", "pair", "pair + drop", "Philox cost", "exact+mask+bmm", "O err"))
    drop = (0.1, 987654321, 5)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(1e3 * a.elapsed_time(b))
        return sorted(ts)[len(ts) // 2]

    for n, k, h, dk in ((8000, 900, 2, 256), (32768, 900, 2, 256), (32768, 500, 4, 192), (32768, 900, 4, 96)):
        g = torch.Generator().manual_seed(n + k)
        d = h * dk
        q, kp, v = (torch.randn(s, d, generator=g).to(dev) for s in (n, k, n))

        def before():
            _, p, _ = ops.sparse_attn_fwd(q, kp, v, h, need_attn=True)
            mask = ops.dropout_mask(h, n, k, *drop, dev)
            return torch.bmm((p * mask).transpose(1, 2), v.reshape(n, h, dk).transpose(0, 1)).transpose(0, 1).reshape(k, d)

        t_plain = timed(lambda: ops.sparse_attn_fwd_x3u(q, kp, v, h, need_attn=True))
        t_drop = timed(lambda: ops.sparse_attn_fwd_x3u(q, kp, v, h, need_attn=True, dropout=drop))
        t_before = timed(before)
        o, p, _ = ops.sparse_attn_fwd_x3u(q, kp, v, h, need_attn=True, dropout=drop)
        err = 0.0
        for a in range(h):                                               # fp64 on the device, a head at a time
            ref = (p[a].double() * ops.dropout_mask(h, n, k, *drop, dev)[a].double()).t() @ v[:, a * dk:(a + 1) * dk].double()
            err = max(err, float((o[:, a * dk:(a + 1) * dk].double() - ref).abs().max() / ref.abs().max()))
        say("%-22s %12.1f %12.1f %12.1f %14.1f %10.2e" % ((n, k, h, dk), t_plain, t_drop, t_drop - t_plain, t_before, err))
        del q, kp, v, o, p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out")
    ap.add_argument("--only", help="'forwards' or 'steps'")
    args = ap.parse_args()
    import torch
    from snuffy_amd import autograd as SA
    from snuffy_amd.train import BagParallelStepper
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

    def window(fn):
        fn()
        t0, n = time.perf_counter(), 0
        while n < 2 or time.perf_counter() - t0 < args.window:
            fn()
            n += 1
        return (time.perf_counter() - t0) / n

    def alternate(fn):
        t = {False: [], True: []}
        for _ in range(args.rounds):
            for on in (False, True):
                SA.X3U_TRAINING = on
                np.random.seed(5)
                torch.manual_seed(5)
                t[on].append(1e3 * window(fn))
        return sorted(t[False]), sorted(t[True])

    def fmt(ts):
        return "%9.3f %9.3f %9.3f" % (ts[0], ts[len(ts) // 2], ts[-1])

    shipped = SA.X3U_TRAINING
    say("fp32 training at head widths 96 / 192 / 256: autograd.X3U_TRAINING on against off, attention dropout 0.1, return_attention off")
    if not args.only or args.only == "forwards":
        say("")
        forwards(say, dev)
    if not args.only or args.only == "steps":
        say("")
        say("ms per optimizer step (min / median / max of %d alternating rounds), peak MB of device memory in a step" % args.rounds)
        say("%-16s %-6s %29s %29s %8s %17s" % ("recipe", "N", "off  min    median       max", "on   min    median       max", "speedup",
                                               "peak MB off -> on"))
        behind_rows = []
        for name, d, h, lam, share, act, depth, enc in RECIPES:
            for n in BAGS:
                x = torch.randn(1, n, d, generator=torch.Generator().manual_seed(7)).to(dev)
                label = torch.tensor([1.0], device=dev)
                st = BagParallelStepper(build_net(dev, d, h, lam, share, act, depth, enc), world_size=1, dist=None, device=dev, precision="fp32")
                peak = {}

                def one():
                    st.step(x, label)
                    torch.cuda.synchronize()

                for on in (False, True):
                    SA.X3U_TRAINING = on
                    one()
                    torch.cuda.reset_peak_memory_stats()
                    one()
                    peak[on] = torch.cuda.max_memory_allocated() / 2 ** 20
                off, on_ = alternate(one)
                sp = off[len(off) // 2] / on_[len(on_) // 2]
                behind = sp < 1.0 and on_[0] > off[-1]
                if behind:
                    behind_rows.append("%s N=%d" % (name, n))
                say("%-16s %-6d %s %s %7.2fx %8.0f -> %-6.0f%s" % (name, n, fmt(off), fmt(on_), sp, peak[False], peak[True],
                                                                  "   BEHIND" if behind else "" if sp >= 1.0 else "   (level: ranges overlap)"))
                del st, x
        say("ship rule (on only if no row is behind outside the spread, and no existing test fails with it on): the timing lets X3U_TRAINING "
            "ship %s%s" % ("OFF" if behind_rows else "ON", (" -- behind at " + ", ".join(behind_rows)) if behind_rows else ""))
    SA.X3U_TRAINING = shipped
    return 0


if __name__ == "__main__":
    sys.exit(main())
