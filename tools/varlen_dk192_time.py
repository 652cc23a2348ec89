"""What packing buys the reference README's MAE recipe (bench.py: readme_mae_adapter D = 768, h = 4, Lambda = 500 as 250 top + 250 random;
dk = 192), whose bf16 bags took the per-bag loop before the dk = 192 attention kernels had varlen forms.

    python tools/varlen_dk192_time.py [--rounds 3] [--window 0.4] [--out profiles/varlen_dk192.txt]

The bf16 model, once with the reference sampler's host draws and once with configure(sampler="device"), return_attention off and on, over
64 bags of 1000 / 8000 patches and a synthetic CAMELYON16-shaped mix (lognormal lengths, sigma 0.5 as balance.py describes the set, median
8000 -- the compositions of tools/varlen_key_chunks_time.py): MILNet.forward_bags with packed.PACK_DK192 on (the packed route) against off
(the routing of before: the per-bag loop, ~25 launches per bag).  A packed launch set holds at most packed.PACK_MAX_ROWS rows: the bags go
to forward_bags in consecutive lists that fit, for both routes alike.  One process; the two routes alternate round by round; every figure
is a host clock around calls that end in a device synchronise, over a window of --window seconds after a warm-up of the same shape."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RECIPE = "readme_mae_adapter"
BAGS = 64


def compositions(lam):
    rs = np.random.RandomState(16)
    mix = np.maximum(np.round(8000 * np.exp(0.5 * rs.randn(BAGS))).astype(int), lam)
    return [("64x1000", [1000] * BAGS), ("64x8000", [8000] * BAGS),
            ("camelyon16_mix(%d..%d)" % (mix.min(), mix.max()), [int(v) for v in mix])]


def launch_lists(sizes, cap):
    out, cur, rows = [], [], 0
    for i, n in enumerate(sizes):
        if cur and rows + n > cap:
            out.append(cur)
            cur, rows = [], 0
        cur.append(i)
        rows += n
    if cur:
        out.append(cur)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.4)
    ap.add_argument("--out")
    ap.add_argument("--only", help="substring of a composition name")
    args = ap.parse_args()
    import torch
    import bench
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

    def run_once(net, lists, bags):
        with torch.no_grad():
            for idx in lists:
                net.forward_bags([bags[i] for i in idx])
        torch.cuda.synchronize()

    def window(net, lists, bags):
        run_once(net, lists, bags)
        t0, n = time.perf_counter(), 0
        while n < 2 or time.perf_counter() - t0 < args.window:
            run_once(net, lists, bags)
            n += 1
        return (time.perf_counter() - t0) / n

    cfg = bench.WORKLOADS[RECIPE]
    say("%s: D = %d, h = %d, Lambda = %d, random share %.2f, bf16; functional.MFMA_ATTN_DK192 = %s (the per-bag loop's attention route)"
        % (RECIPE, cfg["D"], cfg["h"], cfg["lam"], cfg["r"], SF.MFMA_ATTN_DK192))
    say("%d bags per composition; ms per pass over all bags (min / median of %d alternating rounds); slides/s from the median"
        % (BAGS, args.rounds))
    say("%-10s %-5s %-28s %-9s %10s %10s %10s %10s %8s" % ("sampler", "attn", "composition", "packable", "loop min", "loop med",
                                                         "packed min", "packed med", "speedup"))
    net = bench.build_net(cfg["D"], cfg["h"], cfg["lam"], "bf16", dev, cfg["r"]).eval()
    for name, sizes in compositions(cfg["lam"]):
        if args.only and args.only not in name:
            continue
        g = torch.Generator().manual_seed(7)
        bags = [torch.randn(1, n, cfg["D"], generator=g).to(dev) for n in sizes]
        lists = launch_lists(sizes, packed.PACK_MAX_ROWS)
        for sampler in ("reference", "device"):
            for attn in (False, True):
                net.configure(precision="bf16", return_attention=attn, sampler=sampler)
                packed.PACK_DK192 = True
                with torch.no_grad():
                    ok = all(len(idx) > 1 and net._packable([bags[i] for i in idx]) for idx in lists)
                t = {False: [], True: []}
                for _ in range(args.rounds):
                    for on in (False, True):
                        packed.PACK_DK192 = on
                        np.random.seed(5)
                        t[on].append(1e3 * window(net, lists, bags))
                lo, pk = sorted(t[False]), sorted(t[True])
                say("%-10s %-5s %-28s %-9s %10.2f %10.2f %10.2f %10.2f %7.2fx   (%.0f -> %.0f slides/s)" % (
                    sampler, "on" if attn else "off", name, "yes" if ok else "NO", lo[0], lo[len(lo) // 2], pk[0],
                    pk[len(pk) // 2], lo[len(lo) // 2] / pk[len(pk) // 2], 1e3 * BAGS / lo[len(lo) // 2], 1e3 * BAGS / pk[len(pk) // 2]))
        del bags
    return 0


if __name__ == "__main__":
    sys.exit(main())
