"""What the training half of the bf16 MFMA attention at head width 256 buys the reference README's SimCLR ResNet-18 recipe (D = 512, h = 2,
Lambda = 900 as 200 top + 700 random, one encoder layer; dk = 256) at precision="bf16": one optimizer step of train.BagParallelStepper.

    python tools/attn_dk256_train_time.py [--rounds 3] [--window 0.4] [--out profiles/attn_dk256_train.txt]

Two switches of snuffy_amd.autograd, each against the parent's routing (the switch off):
  FUSED_BF16_DK256      ReLU model: the fused first-layer chain (EncoderLayer0Bf16Fn: dropout forward of the width, chunked backward at
                        DK = 256) against the generic autograd chain
  SPARSE_ATTN_FN_WIDE   GELU model (the recipe's activation; the chain declines it): SparseAttnFn on the MFMA kernels -- (q16, kp, v16, lse)
                        saved -- against the exact forward with P and a mask tensor [h, N, K] and the exact backward
at N = 8000 and N = 32768, attention dropout 0.1 (the reference's), encoder dropout off and 0.1.  Kernel-level errors of the backward
first (the figures tests/test_gpu_attn_dk256_train.py bounds).  One process; the two routes alternate round by round; every figure is a
host clock around steps that end in a device synchronise, over a window of --window seconds after a warm-up of the same shape.  The
spread is min / median / max of the rounds; a row is BEHIND when the medians' ratio is under 1 and the ranges do not overlap, LEVEL when
they do (the ship rule: on only if no row is behind outside the run-to-run spread) -- the protocol of tools/attn_dk256_time.py."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, H, LAM, R = 512, 2, 900, 7 / 9
DK = 256


def build_net(dev, act, enc_drop):
    """bench.build_net's initialisation on the recipe's model."""
    import torch
    from snuffy_amd.snuffy import build_milnet
    torch.manual_seed(0)
    net = build_milnet(D, H, act, LAM, R, 1, encoder_dropout=enc_drop)
    for _, p in net.named_parameters():
        if p.dim() > 1:
            torch.nn.init.xavier_normal_(p)
    for m in net.modules():
        if isinstance(m, torch.nn.Linear):
            torch.nn.init.zeros_(m.bias)
    return net.to(dev)


def errors(say, dev):
    """Backward at DK = 256 against fp64 autograd on the bf16-rounded operands (computed on the device), Philox dropout 0.1."""
    import torch
    from snuffy_amd import ops
    say("chunked backward at dk = 256 against fp64 autograd on the bf16-rounded operands, in-kernel dropout 0.1 (bound: 1.5e-2 each)")
    say("%-20s %10s %10s %10s %10s" % ("(n, k, h)", "O rel", "dq rel", "dkp rel", "dv rel"))
    drop = (0.1, 987654321, 5)
    for n, k, h in ((1000, 100, 2), (4100, 129, 2), (2000, 900, 2), (333, 1024, 2)):
        g = torch.Generator().manual_seed(n * 3 + k)
        q, kp, v, dout = (torch.randn(s, h * DK, generator=g).to(dev) for s in (n, k, n, k))
        q16, v16 = q.bfloat16(), v.bfloat16()
        o, _, lse = ops.sparse_attn_fwd_mfma_dk256(q16, v16, kp, h, need_lse=True, dropout=drop)
        dq, dkp, dv = ops.sparse_attn_bwd_mfma(q16, v16, kp, dout, lse, h, dropout=drop)
        mask = ops.dropout_mask(h, n, k, *drop, dev).double()
        qd, kd, vd = (t.bfloat16().double().requires_grad_(True) for t in (q, kp, v))
        qh, kh, vh = (t.view(-1, h, DK).transpose(0, 1) for t in (qd, kd, vd))
        o_r = ((torch.softmax(qh @ kh.transpose(1, 2) / DK ** 0.5, dim=-1) * mask).transpose(1, 2) @ vh).transpose(0, 1).reshape(k, h * DK)
        o_r.backward(dout.bfloat16().double())
        rel = lambda x, y: ((x.double() - y).norm() / y.norm()).item()   # noqa: E731
        say("%-20s %10.3g %10.3g %10.3g %10.3g" % ((n, k, h), rel(o, o_r.detach()), rel(dq, qd.grad), rel(dkp, kd.grad), rel(dv, vd.grad)))
        del q, kp, v, dout, mask, qd, kd, vd, o_r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.4)
    ap.add_argument("--out")
    ap.add_argument("--only", help="'errors', 'chain' or 'generic'")
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

    def alternate(fn, switch):
        t = {False: [], True: []}
        for _ in range(args.rounds):
            for on in (False, True):
                switch(on)
                np.random.seed(5)
                torch.manual_seed(5)
                t[on].append(1e3 * window(fn))
        return sorted(t[False]), sorted(t[True])

    def fmt(ts):
        return "%9.3f %9.3f %9.3f" % (ts[0], ts[len(ts) // 2], ts[-1])

    shipped = (SA.FUSED_BF16_DK256, SA.SPARSE_ATTN_FN_WIDE)
    say("simclr_resnet18 aggregator: D = %d, h = %d, Lambda = %d, random share %.4f, depth 1, precision bf16, one training step" % (D, H, LAM, R))
    if not args.only or args.only == "errors":
        say("")
        errors(say, dev)
    for tag, switch_name, act, what in (("chain", "FUSED_BF16_DK256", "relu", "off = generic autograd chain, on = fused first-layer chain"),
                                        ("generic", "SPARSE_ATTN_FN_WIDE", "gelu", "off = exact kernels with P and a mask tensor, on = MFMA "
                                                                                   "forward with in-kernel dropout + chunked backward")):
        if args.only and args.only != tag:
            continue
        say("")
        say("%s model, ms per optimizer step (min / median / max of %d alternating rounds), peak MB of device memory in a step: %s %s"
            % (act, args.rounds, switch_name, what))
        say("%-8s %-8s %29s %29s %8s %17s" % ("N", "enc drop", "off  min    median       max", "on   min    median       max", "speedup",
                                              "peak MB off -> on"))
        behind_rows = []
        for n in (8000, 32768):
            x = torch.randn(1, n, D, generator=torch.Generator().manual_seed(7)).to(dev)
            label = torch.tensor([1.0], device=dev)
            for enc in (0.0, 0.1):
                st = BagParallelStepper(build_net(dev, act, enc), world_size=1, dist=None, device=dev, precision="bf16")
                peak = {}

                def one():
                    st.step(x, label)
                    torch.cuda.synchronize()

                for on in (False, True):
                    setattr(SA, switch_name, on)
                    one()
                    torch.cuda.reset_peak_memory_stats()
                    one()
                    peak[on] = torch.cuda.max_memory_allocated() / 2 ** 20
                off, on_ = alternate(one, lambda v: setattr(SA, switch_name, v))
                sp = off[len(off) // 2] / on_[len(on_) // 2]
                behind = sp < 1.0 and on_[0] > off[-1]
                if behind:
                    behind_rows.append("N=%d enc drop %.1f" % (n, enc))
                say("%-8d %-8.1f %s %s %7.2fx %8.0f -> %-6.0f%s" % (n, enc, fmt(off), fmt(on_), sp, peak[False], peak[True],
                                                                   "" if behind or sp >= 1.0 else "   (level: ranges overlap)"))
                del st
            del x
        say("ship rule (on only if no row is behind outside the spread, and no existing test fails with it on): the timing lets %s ship %s%s"
            % (switch_name, "OFF" if behind_rows else "ON", (" -- behind at " + ", ".join(behind_rows)) if behind_rows else ""))
    SA.FUSED_BF16_DK256, SA.SPARSE_ATTN_FN_WIDE = shipped
    return 0


if __name__ == "__main__":
    sys.exit(main())
