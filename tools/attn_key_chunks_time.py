"""What the key-chunked MFMA attention backward and the fused bf16 chain above one key chunk gain over the routes such shapes took
before, in THIS tree and -- interleaved, same box, same session -- in another checkout of the project (--other, e.g. the parent commit
built next to this one).

    python tools/attn_key_chunks_time.py [--other PATH] [--series 4] [--steps 16] [--reps 20] [--out FILE]

(a) the attention backward alone at N = 32 768, bf16 operands, attention dropout 0.1, (h, dk, K) in ATTN_SHAPES: ops.sparse_attn_bwd_mfma
    (from the forward's lse and the Philox state) where the tree takes these key counts, and in every tree the exact route the generic
    chain uses there: ops.sparse_attn_bwd with the fp32 P and a mask tensor.
(b) a bf16 training step through BagParallelStepper, attention dropout 0.1, encoder dropout 0 and 0.1, at the shapes of STEP_SHAPES
    (the second is the reference README's first CAMELYON16 recipe: dk = 96, padded), and the config-B step (Lambda = 200, one chunk).

A series is one child process under `timeout`; the trees alternate series by series (this, other, this, ...), timing is by HIP events,
the first child that fails ends the run."""
import argparse
import os
import subprocess
import sys
import time

N = 32768
ATTN_SHAPES = ((4, 128, 500), (4, 128, 900), (6, 64, 500))
# name, D, h, Lambda, random_patch_share
STEP_SHAPES = (("D512_h4_L500", 512, 4, 500, 0.0), ("D384_h4_L900_r7/9", 384, 4, 900, 7.0 / 9.0), ("cfgB_D768_h6_L200", 768, 6, 200, 0.0))
STATE = (0.1, 2 ** 63 + 12345, 2 ** 61 + 77)


def _time(fn, reps):
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.3:                # pre-roll: clocks up, the library's algorithms chosen
        fn()
        torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def attn_leg(root, reps):
    sys.path.insert(0, root)
    import torch
    from snuffy_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    chunked = hasattr(ops, "mfma_attn_train_chunks_supported")
    for h, dk, k in ATTN_SHAPES:
        d = h * dk
        tag = "h%d_dk%d_K%d" % (h, dk, k)
        qv = torch.randn(N, 2 * d, generator=g).to(dev).to(torch.bfloat16)
        q, v = qv[:, :d], qv[:, d:]
        kp = torch.randn(k, d, generator=g).to(dev)
        dout = torch.randn(k, d, generator=g).to(dev)
        # the generic chain's route: fp32 operands, P [h, N, K] from the forward, the mask as a tensor
        qf, vf = q.float(), v.float()
        _, p, lse = ops.sparse_attn_fwd_mfma(q, v, kp, N, h, need_attn=True, need_lse=True)
        mask = ops.dropout_mask(h, N, k, STATE[0], STATE[1], STATE[2], dev)
        ms = _time(lambda: ops.sparse_attn_bwd(qf, kp, vf, p, dout, h, mask=mask), reps)
        print("RESULT what=attn_bwd:%s:exact_P+mask chain=- ms=%.4f" % (tag, ms), flush=True)
        del p, mask, qf, vf
        if chunked:
            ms = _time(lambda: ops.sparse_attn_bwd_mfma(q, v, kp, dout, lse, h, dropout=STATE, fused_bf16_grads=True), reps)
            print("RESULT what=attn_bwd:%s:mfma_chunked chain=- ms=%.4f" % (tag, ms), flush=True)
        del qv, q, v


def step_leg(root, steps):
    sys.path.insert(0, root)
    import torch
    import bench
    from snuffy_amd import autograd as SA
    from snuffy_amd.train import BagParallelStepper
    dev = torch.device("cuda:0")
    for name, D, heads, lam, share in STEP_SHAPES:
        for p in (0.0, 0.1):
            net = bench.build_net(D, heads, lam, "bf16", dev, share)
            layer = net.b_classifier.encoder.layers[0]
            for drop in (layer.sublayer[0].dropout, layer.sublayer[1].dropout, layer.feed_forward.dropout):
                drop.p = p                               # what --encoder_dropout sets; attention dropout stays at its 0.1
            st = BagParallelStepper(net, world_size=1, dist=None, device=dev, precision="bf16")
            g = torch.Generator().manual_seed(1)
            bags = [torch.randn(1, N, D, generator=g).to(dev) for _ in range(2)]
            lab = [torch.tensor([float(i % 2)], device=dev) for i in range(2)]
            calls = []
            real = SA.EncoderLayer0Bf16Fn.apply
            SA.EncoderLayer0Bf16Fn.apply = lambda *a: (calls.append(1), real(*a))[1]
            for i in range(4):
                st.step(bags[i % 2], lab[i % 2])
            torch.cuda.synchronize()
            chain = "fused" if calls else "generic"
            SA.EncoderLayer0Bf16Fn.apply = real
            t0, j = time.perf_counter(), 0
            while time.perf_counter() - t0 < 0.4:
                for _ in range(4):
                    st.step(bags[j % 2], lab[j % 2])
                    j += 1
                torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(steps):
                st.step(bags[i % 2], lab[i % 2])
            e1.record()
            torch.cuda.synchronize()
            print("RESULT what=step:%s:enc_p%.1f chain=%s ms=%.4f" % (name, p, chain, e0.elapsed_time(e1) / steps), flush=True)
            del st, bags, net


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", help="root of another checkout (built) to time against, series interleaved with this tree's")
    ap.add_argument("--series", type=int, default=4)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20, help="launches per figure of the attention backward alone")
    ap.add_argument("--only", choices=("attn", "step"), help="one of the two parts")
    ap.add_argument("--out")
    ap.add_argument("--leg", metavar="ROOT", help="one series of the tree at ROOT, in this process (what the driver starts)")
    ap.add_argument("--part", choices=("attn", "step"))
    args = ap.parse_args()
    if args.leg:
        attn_leg(args.leg, args.reps) if args.part == "attn" else step_leg(args.leg, args.steps)
        return 0
    trees = [("this", here)] + ([("other", os.path.abspath(args.other))] if args.other else [])
    res, chains, lines = {}, {}, []

    def say(s):
        lines.append(s + "\n")
        print(s, flush=True)

    def flush():
        if args.out:
            open(args.out, "w").writelines(lines)

    for part in ("attn", "step"):
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
    say("N = %d, bf16, attention dropout 0.1; %d series, ms per call / per step (fastest and median series per figure)" % (N, args.series))
    for (tag, what), ms in sorted(res.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        srt = sorted(ms)
        med = srt[len(srt) // 2] if len(srt) % 2 else 0.5 * (srt[len(srt) // 2 - 1] + srt[len(srt) // 2])
        say("%-5s %-44s [%-7s]  %s   min %.4f  median %.4f  max %.4f  spread %.2f %%" % (
            tag, what, chains[(tag, what)], "  ".join("%.4f" % v for v in ms), srt[0], med, srt[-1], 100 * (srt[-1] - srt[0]) / srt[0]))
    flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
