"""What encoder dropout costs in the fp32-class training step at config B (N = 32 768, D = 768, h = 6, Lambda = 200, one rank), and what
the fused chain gains over the generic one there: the step with encoder_dropout = 0.1 and with 0, in THIS tree and -- interleaved,
same box, same session -- in another checkout of the project (--other, e.g. the parent commit built next to this one).

    python tools/encoder_dropout_time.py [--other PATH] [--series 5] [--steps 24] [--out FILE]

A series is one child process under `timeout`: it builds the net, warms up, runs an untimed pre-roll and times `steps` back-to-back
steps between two HIP events, for p = 0.1 and then p = 0.  The trees alternate series by series (this, other, this, ...); the first
child that fails ends the run.  A tree whose fused chain declines encoder dropout reports the generic chain for p = 0.1.

    python tools/encoder_dropout_time.py --trace-leg     (under rocprofv3 --kernel-trace --stats: a few p = 0.1 steps, nothing else)"""
import argparse
import os
import subprocess
import sys
import time

D, HEADS, LAM, N = 768, 6, 200, 32768
PS = (0.1, 0.0)


def _net(root, p):
    import torch
    import bench
    from snuffy_amd.train import BagParallelStepper
    dev = torch.device("cuda:0")
    net = bench.build_net(D, HEADS, LAM, "fp32", dev)
    layer = net.b_classifier.encoder.layers[0]
    for drop in (layer.sublayer[0].dropout, layer.sublayer[1].dropout, layer.feed_forward.dropout):
        drop.p = p                                       # what --encoder_dropout sets (snuffy.py:108,225,110); attention dropout stays 0.1
    st = BagParallelStepper(net, world_size=1, dist=None, device=dev, precision="fp32")
    g = torch.Generator().manual_seed(1)
    bags = [torch.randn(1, N, D, generator=g).to(dev) for _ in range(4)]
    lab = [torch.tensor([float(i % 2)], device=dev) for i in range(4)]
    return st, bags, lab


def leg(root, steps):
    sys.path.insert(0, root)
    import torch
    from snuffy_amd import autograd as SA
    for p in PS:
        st, bags, lab = _net(root, p)
        calls = []
        real = SA.EncoderLayer0X3Fn.apply
        SA.EncoderLayer0X3Fn.apply = lambda *a: (calls.append(1), real(*a))[1]
        for i in range(8):
            st.step(bags[i % 4], lab[i % 4])
        torch.cuda.synchronize()
        chain = "fused" if calls else "generic"
        SA.EncoderLayer0X3Fn.apply = real
        t0, j = time.perf_counter(), 0
        while time.perf_counter() - t0 < 0.6:
            for _ in range(8):
                st.step(bags[j % 4], lab[j % 4])
                j += 1
            torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(steps):
            st.step(bags[i % 4], lab[i % 4])
        e1.record()
        torch.cuda.synchronize()
        print("RESULT p=%.1f chain=%s ms_per_step=%.4f" % (p, chain, e0.elapsed_time(e1) / steps), flush=True)
        del st, bags


def trace_leg(root):
    sys.path.insert(0, root)
    import torch
    st, bags, lab = _net(root, 0.1)
    for i in range(12):
        st.step(bags[i % 4], lab[i % 4])
    torch.cuda.synchronize()


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", help="root of another checkout (built) to time against, series interleaved with this tree's")
    ap.add_argument("--series", type=int, default=5)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--out")
    ap.add_argument("--leg", metavar="ROOT", help="one series of the tree at ROOT, in this process (what the driver starts)")
    ap.add_argument("--trace-leg", action="store_true")
    args = ap.parse_args()
    if args.trace_leg:
        trace_leg(here)
        return 0
    if args.leg:
        leg(args.leg, args.steps)
        return 0
    trees = [("this", here)] + ([("other", os.path.abspath(args.other))] if args.other else [])
    res = {(t, p): [] for t, _ in trees for p in PS}
    chains = {}
    lines = []

    def say(s):
        lines.append(s + "\n")
        print(s, flush=True)

    for s in range(args.series):
        for tag, root in trees:
            r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--leg", root, "--steps", str(args.steps)],
                               stdout=subprocess.PIPE, text=True, cwd=root)
            if r.returncode != 0:
                say("series %d of tree %s ended with status %d: stopping" % (s, tag, r.returncode))
                if args.out:
                    open(args.out, "w").writelines(lines)
                return r.returncode
            for line in r.stdout.splitlines():
                if line.startswith("RESULT"):
                    f = dict(kv.split("=") for kv in line.split()[1:])
                    res[(tag, float(f["p"]))].append(float(f["ms_per_step"]))
                    chains[(tag, float(f["p"]))] = f["chain"]
                    say("series %d  %-5s %s" % (s, tag, line[7:]))
    say("")
    say("fp32-class training step, N = %d, D = %d, h = %d, Lambda = %d; %d series of %d steps per figure, ms per step" % (N, D, HEADS, LAM, args.series, args.steps))
    for (tag, p), ms in res.items():
        mean = sum(ms) / len(ms)
        say("%-5s encoder_dropout = %.1f  [%-7s chain]  %s   mean %.4f  min %.4f  max %.4f  spread %.2f %%  %6.1f slides/s" % (
            tag, p, chains[(tag, p)], "  ".join("%.4f" % v for v in ms), mean, min(ms), max(ms), 100 * (max(ms) - min(ms)) / min(ms), 1e3 / mean))
    if args.out:
        open(args.out, "w").writelines(lines)
    return 0


if __name__ == "__main__":
    sys.exit(main())
