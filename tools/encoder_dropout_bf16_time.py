"""What encoder dropout costs in the bf16 training step at config B (N = 32 768, D = 768, h = 6, Lambda = 200, one rank), what the fused
chain gains over the generic one there, and which form of the FFN-in projection with dropout is the faster one: the step with
encoder_dropout = 0.1 and with 0, in THIS tree and -- interleaved, same box, same session -- in another checkout of the project
(--other, e.g. the parent commit built next to this one).

    python tools/encoder_dropout_bf16_time.py [--other PATH] [--series 5] [--steps 24] [--out FILE]
    python tools/encoder_dropout_bf16_time.py --gemm [--other PATH] [--series 3] [--out FILE]

A series is one child process under `timeout`: it builds the net, warms up, runs an untimed pre-roll and times `steps` back-to-back
steps between two HIP events, for p = 0.1 and then p = 0.  The trees alternate series by series (this, other, this, ...); the first
child that fails ends the run.  A tree whose fused chain declines encoder dropout reports the generic chain for p = 0.1.

--gemm: FFN-in of config B (32 768 x 3072 x 768) and of a ViT-S bag (16 384 x 1536 x 384): ops.linear_bf16 without dropout (both trees),
and in this tree the mask in the hand-written GEMM's epilogue, the library GEMM plus the in-place pass, the pass alone, the z assembly
and the dz column-sum pass with dropout next to their dropout-free twins."""
import argparse
import os
import subprocess
import sys
import time

D, HEADS, LAM, N = 768, 6, 200, 32768
PS = (0.1, 0.0)
GEMM_SHAPES = (("cfgB FFN-in", 32768, 3072, 768), ("ViT-S bag FFN-in", 16384, 1536, 384))
STATE = (0.1, 2 ** 63 + 12345, 2 ** 61 + 77)


def _net(p):
    import torch
    import bench
    from snuffy_amd.train import BagParallelStepper
    dev = torch.device("cuda:0")
    net = bench.build_net(D, HEADS, LAM, "bf16", dev)
    layer = net.b_classifier.encoder.layers[0]
    for drop in (layer.sublayer[0].dropout, layer.sublayer[1].dropout, layer.feed_forward.dropout):
        drop.p = p                                       # what --encoder_dropout sets (snuffy.py:108,225,110); attention dropout stays 0.1
    st = BagParallelStepper(net, world_size=1, dist=None, device=dev, precision="bf16")
    g = torch.Generator().manual_seed(1)
    bags = [torch.randn(1, N, D, generator=g).to(dev) for _ in range(4)]
    lab = [torch.tensor([float(i % 2)], device=dev) for i in range(4)]
    return st, bags, lab


def leg(root, steps):
    sys.path.insert(0, root)
    import torch
    from snuffy_amd import autograd as SA
    for p in PS:
        st, bags, lab = _net(p)
        calls = []
        real = SA.EncoderLayer0Bf16Fn.apply
        SA.EncoderLayer0Bf16Fn.apply = lambda *a: (calls.append(1), real(*a))[1]
        for i in range(8):
            st.step(bags[i % 4], lab[i % 4])
        torch.cuda.synchronize()
        chain = "fused" if calls else "generic"
        SA.EncoderLayer0Bf16Fn.apply = real
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
        print("RESULT what=step_p%.1f chain=%s ms=%.4f" % (p, chain, e0.elapsed_time(e1) / steps), flush=True)
        del st, bags


def _time(fn, reps):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.3:                # pre-roll: clocks up, the library's algorithm chosen
        for _ in range(4):
            fn()
        torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def gemm_leg(root, reps):
    sys.path.insert(0, root)
    import torch
    from snuffy_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(2)
    new = hasattr(ops, "linear_bf16_dropout")
    for tag, m, n, k in GEMM_SHAPES:
        key = tag.split()[0]
        a = torch.randn(m, k, generator=g).to(dev).to(torch.bfloat16)
        w = (torch.randn(n, k, generator=g) / k ** 0.5).to(dev).to(torch.bfloat16)
        b = torch.randn(n, generator=g).to(dev)
        bh = b.to(torch.bfloat16)
        legs = [("linear_bf16[%s]" % ("native" if ops.gemm_prefers_native(m, n, k) else "library"), lambda: ops.linear_bf16(a, w, b, bh, "relu")),
                ("plain_native", lambda: ops.linear_bf16(a, w, b, bh, "relu", prefer_native=True)),
                ("plain_library", lambda: ops.linear_bf16(a, w, b, bh, "relu", prefer_native=False))]
        if new:
            hid = ops.linear_bf16(a, w, b, bh, "relu")
            legs += [("drop_native", lambda: ops.linear_bf16_dropout(a, w, b, bh, STATE, prefer_native=True)),
                     ("drop_library+pass", lambda: ops.linear_bf16_dropout(a, w, b, bh, STATE, prefer_native=False)),
                     ("drop_routed[%s]" % ("native" if ops.dropout_gemm_prefers_native(m, n, k) else "library+pass"),
                      lambda: ops.linear_bf16_dropout(a, w, b, bh, STATE)),
                     ("pass_alone", lambda: ops.dropout_rows_bf16_(hid, STATE))]
        for name, fn in legs:
            print("RESULT what=%s:%s chain=- ms=%.4f" % (key, name, _time(fn, reps)), flush=True)
        del a, w, legs
    if new:                                              # the two other passes at config B's z / dz
        from snuffy_amd import functional as SF
        x = torch.randn(N, D, generator=g).to(dev)
        zb = torch.randn(N, D, generator=g).to(dev).to(torch.bfloat16)
        b2 = torch.randn(D, generator=g).to(dev)
        sel = torch.randperm(N, generator=g)[:LAM].to(dev)
        slot, delta = ops.slot_map(sel, N), torch.randn(LAM, D, generator=g).to(dev)
        parts = SF.Parts(x, add_bf16=zb, add_bias=b2, slot=slot, delta=delta)
        for name, fn in (("z_materialize", lambda: SF.materialize(parts)),
                         ("z_assemble_dropout", lambda: ops.residual_assemble_dropout(x, zb, b2, slot, delta, STATE)),
                         ("dz_colsum", lambda: ops.colsum_fused(x, want_bf16=True)),
                         ("dz_colsum_dropout", lambda: ops.colsum_fused(x, want_bf16=True, dropout=STATE))):
            print("RESULT what=cfgB:%s chain=- ms=%.4f" % (name, _time(fn, reps)), flush=True)


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", help="root of another checkout (built) to time against, series interleaved with this tree's")
    ap.add_argument("--series", type=int, default=5)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--reps", type=int, default=40, help="--gemm: launches per figure")
    ap.add_argument("--gemm", action="store_true", help="the FFN-in forms and the two passes instead of the step")
    ap.add_argument("--out")
    ap.add_argument("--leg", metavar="ROOT", help="one series of the tree at ROOT, in this process (what the driver starts)")
    args = ap.parse_args()
    if args.leg:
        gemm_leg(args.leg, args.reps) if args.gemm else leg(args.leg, args.steps)
        return 0
    trees = [("this", here)] + ([("other", os.path.abspath(args.other))] if args.other else [])
    res, chains, lines = {}, {}, []

    def say(s):
        lines.append(s + "\n")
        print(s, flush=True)

    for s in range(args.series):
        for tag, root in trees:
            cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--leg", root, "--steps", str(args.steps),
                   "--reps", str(args.reps)] + (["--gemm"] if args.gemm else [])
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, cwd=root)
            if r.returncode != 0:
                say("series %d of tree %s ended with status %d: stopping" % (s, tag, r.returncode))
                if args.out:
                    open(args.out, "w").writelines(lines)
                return r.returncode
            for line in r.stdout.splitlines():
                if line.startswith("RESULT"):
                    f = dict(kv.split("=", 1) for kv in line.split()[1:])
                    res.setdefault((tag, f["what"]), []).append(float(f["ms"]))
                    chains[(tag, f["what"])] = f["chain"]
                    say("series %d  %-5s %s" % (s, tag, line[7:]))
    say("")
    if args.gemm:
        say("FFN-in with encoder dropout, bf16; %d series of %d launches per figure, ms per call" % (args.series, args.reps))
    else:
        say("bf16 training step, N = %d, D = %d, h = %d, Lambda = %d; %d series of %d steps per figure, ms per step" % (N, D, HEADS, LAM, args.series, args.steps))
    for (tag, what), ms in res.items():
        mean = sum(ms) / len(ms)
        say("%-5s %-34s [%-7s]  %s   mean %.4f  min %.4f  max %.4f  spread %.2f %%%s" % (
            tag, what, chains[(tag, what)], "  ".join("%.4f" % v for v in ms), mean, min(ms), max(ms), 100 * (max(ms) - min(ms)) / min(ms),
            "" if args.gemm else "  %6.1f slides/s" % (1e3 / mean)))
    if args.out:
        open(args.out, "w").writelines(lines)
    return 0


if __name__ == "__main__":
    sys.exit(main())
