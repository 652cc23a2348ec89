"""What a bag length off gemm_tn's 32-row grid costs: the training step (fp32-class and bf16, D = 768, h = 6, Lambda = 200, one rank) at
N = 32 768 and at N = 32 749, and ops.gemm_tn alone on the three weight-gradient shapes of that step at both lengths, plane and hl
images.  Every timed figure is a region of back-to-back launches between two HIP events, behind warm-up steps and an untimed pre-roll;
REGIONS regions per figure, so that the spread of the box stands next to every comparison.

    python tools/train_row_tail_time.py [--out FILE]

Each leg runs in a child process of its own under `timeout`; the first leg that fails ends the run.  A tree whose gemm_tn takes whole
steps only reports "unsupported" for the lone contraction at N = 32 749 and times its fallback chain in the training legs."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LENGTHS = (32768, 32749)
SHAPES = ((768, 3072), (3072, 768), (1536, 768))
D, HEADS, LAM = 768, 6, 200
REGIONS = 4
LEGS = (("train", "fp32", 420), ("train", "bf16", 300), ("tn", "-", 300))


def _regions(fn, per_region, preroll_s):
    """ms per call of fn(i) in each of REGIONS event-timed regions of per_region calls, behind an untimed pre-roll."""
    import torch
    t0, j = time.perf_counter(), 0
    while time.perf_counter() - t0 < preroll_s:
        for _ in range(8):
            fn(j)
            j += 1
        torch.cuda.synchronize()
    out = []
    for _ in range(REGIONS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(per_region):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / per_region)
    return out


def _fmt(ms):
    return "  ".join("%8.4f" % v for v in ms) + "   (min %.4f  max %.4f  spread %.2f %%)" % (min(ms), max(ms), 100 * (max(ms) - min(ms)) / min(ms))


def leg_train(precision):
    import torch
    import bench
    from snuffy_amd import autograd as SA
    from snuffy_amd import ops
    from snuffy_amd.train import BagParallelStepper
    dev = torch.device("cuda:0")
    for n in LENGTHS:
        net = bench.build_net(D, HEADS, LAM, precision, dev)
        st = BagParallelStepper(net, world_size=1, dist=None, device=dev, precision=precision)
        g = torch.Generator().manual_seed(1)
        bags = [torch.randn(1, n, D, generator=g).to(dev) for _ in range(4)]
        lab = [torch.tensor([float(i % 2)], device=dev) for i in range(4)]
        for i in range(8):
            st.step(bags[i % 4], lab[i % 4])
        torch.cuda.synchronize()
        ms = _regions(lambda i: st.step(bags[i % 4], lab[i % 4]), 24, 0.6)
        chain = ("one-pass hl chain" if SA._x3_train_hl_ok(n, D, 4 * D) else "concatenated-K chain") if precision == "fp32" else \
            ("gemm_tn contractions" if ops.gemm_tn_supported(n, D, 4 * D) else "library contractions")
        print("train %-4s N=%5d  ms/step %s  %6.1f slides/s at the fastest  [%s]" % (precision, n, _fmt(ms), 1e3 / min(ms), chain), flush=True)
        del st, net, bags


def leg_tn():
    import torch
    from snuffy_amd import ops
    dev = "cuda:0"
    for p, q in SHAPES:
        for layout in ("x3", "hl", "bf16"):
            for n in LENGTHS:
                g = torch.Generator().manual_seed(n + p + q)
                a, b = torch.randn(n, p, generator=g).to(dev), torch.randn(n, q, generator=g).to(dev)
                if layout == "x3":
                    a_img, b_img, kw = ops.split3_rows(a), ops.split3_rows(b), dict(a_planes=(p, 2 * p), b_planes=(q, 2 * q))
                elif layout == "hl":
                    a_img, b_img, kw = ops.split_hl_rows(a), ops.split_hl_rows(b), dict(hl=True)
                else:
                    a_img, b_img, kw = a.to(torch.bfloat16), b.to(torch.bfloat16), {}
                del a, b
                out = torch.empty(p, q, device=dev)
                tag = "gemm_tn %-4s %4d x %4d N=%5d" % (layout, p, q, n)
                try:
                    ops.gemm_tn(a_img, b_img, p, q, out=out, **kw)
                except ValueError:
                    print("%s  unsupported" % tag, flush=True)
                    continue
                torch.cuda.synchronize()
                ms = _regions(lambda i: ops.gemm_tn(a_img, b_img, p, q, out=out, **kw), 50, 0.3)
                print("%s  ms/call %s" % (tag, _fmt(ms)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", nargs=2, metavar=("KIND", "PRECISION"), help="run one leg in this process (what the driver starts)")
    ap.add_argument("--out", help="also write the lines to this file")
    args = ap.parse_args()
    if args.leg:
        if args.leg[0] == "train":
            leg_train(args.leg[1])
        else:
            leg_tn()
        return 0
    lines = []
    for kind, precision, limit in LEGS:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--leg", kind, precision],
                           stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        lines.append(r.stdout)
        if r.returncode != 0:
            lines.append("leg %s %s ended with status %d: stopping\n" % (kind, precision, r.returncode))
            sys.stdout.write(lines[-1])
            break
    if args.out:
        with open(args.out, "w") as fh:
            fh.writelines(lines)
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
