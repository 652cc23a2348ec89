#!/usr/bin/env python3
"""ResNet-18 (InstanceNorm) patch extractor: throughput of snuffy_amd.resnet against a plain-torch restatement of the same network
(F.conv2d / F.instance_norm, channels-last, fp32 and bf16 autocast -- what a user would run without this package), in one process, in
alternating rounds; time per kernel form from HIP events with the FLOPs computed from the shapes; the bf16 error figures of
tests/test_gpu_resnet.py.

usage: python tools/bench_resnet.py [--batch 512] [--size 224] [--rounds 5] [--iters 3] [--no-errors]"""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from snuffy_amd import ops  # noqa: E402
from snuffy_amd.resnet import ResNet18  # noqa: E402

DEV = "cuda"


def torch_forward(sd, x):
    """torchvision's resnet18 forward (norm_layer = InstanceNorm2d, fc = Identity) on a state dict."""
    def block(t, p, stride):
        y = torch.relu(F.instance_norm(F.conv2d(t, sd[p + ".conv1.weight"], stride=stride, padding=1)))
        y = F.instance_norm(F.conv2d(y, sd[p + ".conv2.weight"], padding=1))
        if p + ".downsample.0.weight" in sd:
            t = F.instance_norm(F.conv2d(t, sd[p + ".downsample.0.weight"], stride=stride))
        return torch.relu(y + t)

    t = F.max_pool2d(torch.relu(F.instance_norm(F.conv2d(x, sd["conv1.weight"], stride=2, padding=3))), 3, 2, 1)
    for layer in (1, 2, 3, 4):
        t = block(t, "layer%d.0" % layer, 1 if layer == 1 else 2)
        t = block(t, "layer%d.1" % layer, 1)
    return t.mean((2, 3))


def conv_shapes(size):
    """[(label, cin, cout, k, stride, input side, count in the network)] and the network's FLOPs per image (2 per multiply-add)."""
    out = lambda n, k, s: (n + 2 * (k // 2) - k) // s + 1
    side = out(size, 7, 2)
    shapes = [("stem 7x7/2 3->64", 3, 64, 7, 2, size, 1)]
    side = out(side, 3, 2)
    cin = 64
    for planes in (64, 128, 256, 512):
        if planes != 64:
            shapes.append(("3x3/2 %d->%d" % (cin, planes), cin, planes, 3, 2, side, 1))
            shapes.append(("1x1/2 %d->%d" % (cin, planes), cin, planes, 1, 2, side, 1))
            side = out(side, 3, 2)
        shapes.append(("3x3/1 %d->%d" % (planes, planes), planes, planes, 3, 1, side, 4 if planes == 64 else 3))
        cin = planes
    flops = sum(n * 2 * out(s, k, st) ** 2 * co * ci * k * k for _, ci, co, k, st, s, n in shapes)
    return shapes, flops


def timed(fn, iters):
    """milliseconds per call, HIP events around `iters` calls."""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def kernel_forms(size, batch, iters):
    shapes, _ = conv_shapes(size)
    print("# time per kernel form, batch %d (one pass of the module), HIP events, %d calls each" % (batch, iters))
    for label, cin, cout, k, stride, side, count in shapes:
        w = torch.randn(cout, cin, k, k, device=DEV) * 0.05
        for prec in ("fp32-class", "bf16"):
            hi, lo = ops.conv_pack_weight(w, split=prec == "fp32-class", kp=ops.CONV_STEM_KP if k == 7 else None)
            if k == 7:
                x = torch.rand(batch, 3, side, side, device=DEV)
                ms = timed(lambda: ops.conv_stem(x, hi, lo), iters)
                ho = ops.conv2d_plan(batch, side, side, 3, 64, 7, 2)[0]
            else:
                x = torch.rand(batch, side, side, cin, device=DEV)
                if prec == "bf16":
                    x = x.to(torch.bfloat16)
                ms = timed(lambda: ops.conv2d_nhwc(x, hi, lo, k, stride), iters)
                ho = ops.conv2d_plan(batch, side, side, cin, cout, k, stride)[0]
            fl = 2.0 * batch * ho * ho * cout * cin * k * k
            print("conv %-18s in %3dx%-3d x%d  %-10s %8.3f ms  %7.1f TFLOP/s (useful)" % (label, side, side, count, prec, ms, fl / ms * 1e-9))
            del x
    for side, c in ((112, 64), (56, 64), (28, 128), (14, 256), (7, 512)):
        if size != 224:
            break
        y = torch.randn(batch, side, side, c, device=DEV)
        ms_s = timed(lambda: ops.instnorm_stats_nhwc(y), iters)
        mean, rstd = ops.instnorm_stats_nhwc(y)
        ms_n = timed(lambda: ops.norm_act_nhwc(y, mean, rstd, None, None, y, True), iters)
        gb = y.numel() * 4e-9
        print("instnorm_stats %3dx%-3d c%-3d %8.3f ms  %6.0f GB/s (two reads) | norm_act + identity + relu %8.3f ms  %6.0f GB/s" % (
            side, side, c, ms_s, 2 * gb / ms_s * 1e3, ms_n, 3 * gb / ms_n * 1e3))
        if side == 112:
            ms = timed(lambda: ops.maxpool3x3s2_nhwc(y), iters)
            print("maxpool3x3s2  112x112 c64  %8.3f ms" % ms)
        if side == 7:
            ms = timed(lambda: ops.avgpool_nhwc(y), iters)
            print("avgpool         7x7   c512 %8.3f ms" % ms)
        del y


def errors():
    """bf16 rel_err (max |a - b| / max |b|) against fp64 of the package and of the emulation that rounds only the two operands of every
    convolution to bf16 -- the three figures of tests/test_gpu_resnet.py::test_model_bf16."""
    from tests import test_gpu_resnet as T
    print("# bf16 features against fp64 (B = 2, the inputs and weights of tests/test_gpu_resnet.py)")
    for h, w in ((64, 64), (72, 88), (224, 224)):
        model, x, ref, emu = T.model_case("instance", h, w)
        out = model.configure("bf16")(x.to(DEV))
        f32 = model.configure("fp32")(x.to(DEV))
        print("%3dx%-3d  package bf16 rel_err %.3e | all-conv bf16 emulation %.3e | package fp32 class max abs err %.3e" % (
            h, w, T.rel_err(out.cpu(), ref), T.rel_err(emu, ref), float((f32.cpu().double() - ref).abs().max())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--no-errors", action="store_true")
    ap.add_argument("--no-forms", action="store_true")
    args = ap.parse_args()
    torch.manual_seed(0)
    model = ResNet18("instance").to(DEV).eval()
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    sd_cl = {k: v.contiguous(memory_format=torch.channels_last) for k, v in sd.items()}
    x = torch.rand(args.batch, 3, args.size, args.size, device=DEV)
    x_cl = x.contiguous(memory_format=torch.channels_last)
    _, flops = conv_shapes(args.size)
    print("# %s | torch %s | batch %d at %dx%d | %.3f GFLOP per image in the convolutions" % (
        torch.cuda.get_device_name(0), torch.__version__, args.batch, args.size, args.size, flops * 1e-9))

    def run_torch_bf16():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return torch_forward(sd_cl, x_cl)

    variants = [("snuffy_amd fp32 class", lambda: model.configure("fp32")(x)),
                ("snuffy_amd bf16", lambda: model.configure("bf16")(x)),
                ("torch fp32 channels-last", lambda: torch_forward(sd_cl, x_cl)),
                ("torch bf16 autocast channels-last", run_torch_bf16)]
    times = {name: [] for name, _ in variants}
    with torch.no_grad():
        for name, fn in variants:           # warm-up: weight images, library kernel selection
            fn()
            fn()
        torch.cuda.synchronize()
        for _ in range(args.rounds):        # alternating rounds: every variant sees the same clocks and temperature
            for name, fn in variants:
                times[name].append(timed(fn, args.iters))
        print("# whole network, %d alternating rounds of %d forwards: median [min .. max] ms per batch, img/s at the median" % (
            args.rounds, args.iters))
        for name, _ in variants:
            t = times[name]
            med = statistics.median(t)
            print("%-36s %9.2f [%9.2f .. %9.2f] ms  %8.0f img/s  %6.1f TFLOP/s (useful)" % (
                name, med, min(t), max(t), args.batch / med * 1e3, flops * args.batch / med * 1e-9))
        a = model.configure("fp32")(x[:8])
        b = torch_forward(sd, x[:8])
        print("# fp32 class against torch fp32 on 8 images: max abs diff %.3e" % float((a - b).abs().max()))
        if not args.no_forms:
            kernel_forms(args.size, min(args.batch, model.max_batch), max(args.iters, 5))
        if not args.no_errors:
            errors()
    print("# done %s" % time.strftime("%Y-%m-%d"))


if __name__ == "__main__":
    main()
