"""What the bf16 MFMA attention kernel at head width 256 buys the reference README's SimCLR ResNet-18 recipe (D = 512, h = 2, Lambda = 900
as 200 top + 700 random, gelu, one encoder layer; dk = 256) at precision="bf16", single bag and packed.

    python tools/attn_dk256_time.py [--rounds 3] [--window 0.4] [--out profiles/attn_dk256.txt]

Errors first: the single-bag entry point on a few (n, k, h) against fp64 on the exact and on the bf16-rounded operands (the figures
tests/test_gpu_attn_dk256.py::test_forward bounds).
Single bag: one forward at N = 8000 / 32768 with functional.MFMA_ATTN_DK256 on (the bf16 kernel of the width) against off (the routing of
before: fp32 copies of Q | V into the exact-fp32 kernel), return_attention off and on.  Packed: MILNet.forward_bags with packed.PACK_DK256 on
(the packed route) against off (the per-bag loop, whose attention is the single-bag route that the first section's rule ships), once with the reference sampler's
host draws and once with configure(sampler="device"), return_attention off and on, over 64 bags of 1000 / 8000 patches and a synthetic
CAMELYON16-shaped mix (the compositions of tools/varlen_dk192_time.py).  A packed launch set holds at most packed.PACK_MAX_ROWS rows: the
bags go to forward_bags in consecutive lists that fit, for both routes alike.  One process; the two routes alternate round by round;
every figure is a host clock around calls that end in a device synchronise, over a window of --window seconds after a warm-up of the same
shape.  The spread is min / median / max of the rounds; a row is BEHIND when the medians' ratio is under 1 and LEVEL when the two routes'
min .. max ranges overlap (the ship rule: on only if no row is behind outside the run-to-run spread)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

D, H, LAM, R, ACT = 512, 2, 900, 7 / 9, "gelu"
DK = 256


def build_net(dev):
    """bench.build_net's initialisation on the recipe's model (bench.py builds ReLU models only)."""
    import torch
    from snuffy_amd.snuffy import build_milnet
    torch.manual_seed(0)
    net = build_milnet(D, H, ACT, LAM, R, 1)
    for _, p in net.named_parameters():
        if p.dim() > 1:
            torch.nn.init.xavier_normal_(p)
    for m in net.modules():
        if isinstance(m, torch.nn.Linear):
            torch.nn.init.zeros_(m.bias)
    return net.to(dev).configure(precision="bf16", return_attention=False)


def errors(say, dev):
    """Kernel-level errors against fp64 (computed on the device)."""
    import torch
    from snuffy_amd import ops

    def ref(q, kp, v, h):
        n, k = q.shape[0], kp.shape[0]
        qh, kh, vh = (t.double().view(-1, h, DK).transpose(0, 1) for t in (q, kp, v))
        s = qh @ kh.transpose(1, 2) / DK ** 0.5
        p = torch.softmax(s, dim=-1)
        return (p.transpose(1, 2) @ vh).transpose(0, 1).reshape(k, h * DK), p, torch.logsumexp(s, -1)

    say("single-bag kernel against fp64: exact operands | bf16-rounded operands (bounds: P 1e-2, O 1e-2 | P 2e-5 + 2e-3 max P, O 3e-3, lse 1e-3)")
    say("%-20s %10s %10s %10s %10s %10s %10s" % ("(n, k, h)", "|dP|", "O rel", "|dP| r", "max P", "O rel r", "|dlse| r"))
    for n, k, h in ((1000, 100, 2), (4100, 129, 2), (2000, 900, 2), (333, 1024, 2), (40000, 200, 2)):
        g = torch.Generator().manual_seed(n * 3 + k)
        q, kp, v = (torch.randn(s, h * DK, generator=g).to(dev) for s in (n, k, n))
        o, a, l = ops.sparse_attn_fwd_mfma_dk256(q.bfloat16(), v.bfloat16(), kp, h, need_attn=True, need_lse=True)
        rel = lambda x, y: ((x.double() - y).norm() / y.norm()).item()   # noqa: E731
        o0, p0, _ = ref(q, kp, v, h)
        o1, p1, l1 = ref(q.bfloat16().float(), kp.bfloat16().float(), v.bfloat16().float(), h)
        say("%-20s %10.3g %10.3g %10.3g %10.3g %10.3g %10.3g" % ((n, k, h), (a.double() - p0).abs().max().item(), rel(o, o0),
                                                               (a.double() - p1).abs().max().item(), p1.max().item(), rel(o, o1),
                                                               (l.double() - l1).abs().max().item()))
        del q, kp, v, o, a, l, o0, p0, o1, p1, l1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.4)
    ap.add_argument("--out")
    ap.add_argument("--only", help="substring of a row name ('errors', 'single', or of a composition)")
    args = ap.parse_args()
    import torch
    from varlen_dk192_time import BAGS, compositions, launch_lists
    from snuffy_amd import functional as SF
    from snuffy_amd import packed
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

    def alternate(fn, switch):
        """ms per call of fn() with switch(False) / switch(True), alternating round by round: {flag: sorted times}"""
        t = {False: [], True: []}
        for _ in range(args.rounds):
            for on in (False, True):
                switch(on)
                np.random.seed(5)
                t[on].append(1e3 * window(fn))
        return sorted(t[False]), sorted(t[True])

    def fmt(ts):
        return "%9.3f %9.3f %9.3f" % (ts[0], ts[len(ts) // 2], ts[-1])

    def verdict(old, new):
        """(speedup of the medians, behind outside the spread?)"""
        sp = old[len(old) // 2] / new[len(new) // 2]
        return sp, sp < 1.0 and new[0] > old[-1]

    shipped = (SF.MFMA_ATTN_DK256, packed.PACK_DK256)
    say("simclr_resnet18 aggregator: D = %d, h = %d, Lambda = %d, random share %.4f, %s, depth 1, precision bf16" % (D, H, LAM, R, ACT))
    net = build_net(dev).eval()
    if not args.only or args.only in "errors":
        say("")
        errors(say, dev)

    # ---- single bag: functional.MFMA_ATTN_DK256 ------------------------------------------------------------------------------------
    single = not (args.only and args.only not in "single")
    behind_single = []
    if single:
        say("")
        say("single bag, ms per forward (min / median / max of %d alternating rounds): MFMA_ATTN_DK256 off = fp32 copies into the exact "
            "kernel, on = bf16 kernel" % args.rounds)
        say("%-8s %-5s %29s %29s %8s" % ("N", "attn", "off  min    median       max", "on   min    median       max", "speedup"))
    for n in (8000, 32768):
        if not single:
            continue
        x = torch.randn(1, n, D, generator=torch.Generator().manual_seed(7)).to(dev)
        for attn in (False, True):
            net.configure(precision="bf16", return_attention=attn, sampler="reference")

            def one():
                with torch.no_grad():
                    net(x)
                torch.cuda.synchronize()

            off, on = alternate(one, lambda v: setattr(SF, "MFMA_ATTN_DK256", v))
            sp, behind = verdict(off, on)
            if behind:
                behind_single.append("N=%d attn %s" % (n, "on" if attn else "off"))
            say("%-8d %-5s %s %s %7.2fx%s" % (n, "on" if attn else "off", fmt(off), fmt(on), sp,
                                              "" if behind or sp >= 1.0 else "   (level: ranges overlap)"))
        del x
    if single:
        say("ship rule (on only if no row is behind outside the spread): MFMA_ATTN_DK256 ships %s%s"
            % ("OFF" if behind_single else "ON", (" -- behind at " + ", ".join(behind_single)) if behind_single else ""))
    # the loop the packed route is held against runs the single-bag route that the rule above ships (the faster loop where it is on)
    SF.MFMA_ATTN_DK256 = (not behind_single) if single else shipped[0]

    # ---- packed: packed.PACK_DK256 ----------------------------------------------------------------------------------------------------
    say("")
    say("packed, %d bags per composition; ms per pass over all bags (min / median / max of %d alternating rounds); PACK_DK256 off = "
        "per-bag loop (with MFMA_ATTN_DK256 %s), on = packed route; slides/s from the median"
        % (BAGS, args.rounds, "on" if SF.MFMA_ATTN_DK256 else "off"))
    say("%-10s %-5s %-28s %-9s %29s %29s %8s" % ("sampler", "attn", "composition", "packable", "loop min    median       max",
                                                "packed min  median       max", "speedup"))
    behind_packed, rows_done = [], 0
    for name, sizes in compositions(LAM):
        if args.only and args.only not in name:
            continue
        g = torch.Generator().manual_seed(7)
        bags = [torch.randn(1, n, D, generator=g).to(dev) for n in sizes]
        lists = launch_lists(sizes, packed.PACK_MAX_ROWS)

        def one_pass():
            with torch.no_grad():
                for idx in lists:
                    net.forward_bags([bags[i] for i in idx])
            torch.cuda.synchronize()

        for sampler in ("reference", "device"):
            for attn in (False, True):
                net.configure(precision="bf16", return_attention=attn, sampler=sampler)
                packed.PACK_DK256 = True
                with torch.no_grad():
                    ok = all(len(idx) > 1 and net._packable([bags[i] for i in idx]) for idx in lists)
                lo, pk = alternate(one_pass, lambda v: setattr(packed, "PACK_DK256", v))
                sp, behind = verdict(lo, pk)
                rows_done += 1
                if behind:
                    behind_packed.append("%s %s attn %s" % (name, sampler, "on" if attn else "off"))
                say("%-10s %-5s %-28s %-9s %s %s %7.2fx   (%.0f -> %.0f slides/s)%s" % (
                    sampler, "on" if attn else "off", name, "yes" if ok else "NO", fmt(lo), fmt(pk), sp,
                    1e3 * BAGS / lo[len(lo) // 2], 1e3 * BAGS / pk[len(pk) // 2], "" if behind or sp >= 1.0 else "   (level: ranges overlap)"))
        del bags
    SF.MFMA_ATTN_DK256, packed.PACK_DK256 = shipped
    if rows_done:
        say("ship rule (on only if no row is behind outside the spread): PACK_DK256 ships %s%s"
            % ("OFF" if behind_packed else "ON", (" -- behind at " + ", ".join(behind_packed)) if behind_packed else ""))
    return 0


if __name__ == "__main__":
    sys.exit(main())
