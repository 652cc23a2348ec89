"""What drawing the random patch share on the device buys MILNet.forward_bags on the reference README's two DINO recipes (bench.py:
readme_dino_scratch D = 384, h = 4, Lambda = 900, share 7/9; readme_dino_adapter Lambda = 500, share 0.5).

    python tools/packed_sampler_time.py [--rounds 3] [--window 0.3] [--out profiles/packed_device_sampler.txt]

For both recipes, both precisions (return_attention off, as the validation loop of train.py runs it) and 64 bags of 1000 / 8000 patches
plus the synthetic CAMELYON16-shaped mix of tools/varlen_key_chunks_time.py: forward_bags under sampler="reference" (a device -> host
copy of the top rows, then one np.random.choice per bag and layer), under sampler="device" issued eagerly (one draw launch per group)
and under sampler="device" with graph_max_patches (replay).  The bags go to forward_bags in consecutive lists of at most
packed.PACK_MAX_ROWS rows, the same lists for the three settings.  One process; the settings alternate round by round; every figure is
a host clock around calls that end in a device synchronise, over a window of --window seconds after warm-up passes of the same shape
(three, so that a graph is captured before its window opens).  spread = (max - min) / median over the rounds of a setting."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

RECIPES = ("readme_dino_scratch", "readme_dino_adapter")
SETTINGS = ("reference", "device", "device+graph")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--out")
    ap.add_argument("--only", help="substring of a composition name")
    args = ap.parse_args()
    import torch
    import bench
    from snuffy_amd import packed
    from varlen_key_chunks_time import BAGS, compositions, launch_lists
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
        for _ in range(3):
            run_once(net, lists, bags)
        t0, n = time.perf_counter(), 0
        while n < 2 or time.perf_counter() - t0 < args.window:
            run_once(net, lists, bags)
            n += 1
        return (time.perf_counter() - t0) / n

    def setting(net, precision, name):
        net.configure(precision=precision, return_attention=False, sampler="reference" if name == "reference" else "device",
                      graph_max_patches=(1 << 20) if name.endswith("graph") else 0)

    packed.PACK_DEVICE_SAMPLER = True
    say("%d bags per composition; ms per pass over all bags: min / median of %d alternating rounds, spread = (max - min) / median"
        % (BAGS, args.rounds))
    say("%-20s %-5s %-28s " % ("recipe", "prec", "composition") + " ".join("%-26s" % s for s in SETTINGS) + " ref/device  ref/graph")
    for recipe in RECIPES:
        cfg = bench.WORKLOADS[recipe]
        for precision in ("fp32", "bf16"):
            net = bench.build_net(cfg["D"], cfg["h"], cfg["lam"], precision, dev, cfg["r"]).eval()
            for name, sizes in compositions(cfg["lam"]):
                if name == "64x2000" or (args.only and args.only not in name):
                    continue
                g = torch.Generator().manual_seed(7)
                bags = [torch.randn(1, n, cfg["D"], generator=g).to(dev) for n in sizes]
                lists = launch_lists(sizes, packed.PACK_MAX_ROWS)
                t = {s: [] for s in SETTINGS}
                for _ in range(args.rounds):
                    for s in SETTINGS:
                        setting(net, precision, s)
                        np.random.seed(5)
                        t[s].append(1e3 * window(net, lists, bags))
                        net.configure(graph_max_patches=0)           # drops the captured graphs and their packed buffers
                med = {s: sorted(v)[len(v) // 2] for s, v in t.items()}
                cols = " ".join("%7.2f /%7.2f  (%4.1f %%) " % (min(t[s]), med[s], 100 * (max(t[s]) - min(t[s])) / med[s]) for s in SETTINGS)
                say("%-20s %-5s %-28s %s %9.2fx %9.2fx" % (recipe, precision, name, cols, med["reference"] / med["device"],
                                                          med["reference"] / med["device+graph"]))
                del bags
            del net
    return 0


if __name__ == "__main__":
    sys.exit(main())
