"""What the training augmentations cost on the device (snuffy_amd/augment.py, csrc/augment.hip).

    python tools/augment_time.py [--window 0.5] [--rounds 3] [--cpu-crops 40] [--out profiles/augment.txt]

DINOAugment (2 x 224 + 8 x 96 views) on 64 and on 512 decoded tiles of 256 x 256, MAEAugment (1 x 224) on 64 tiles: ms per batch and
crops / s from device events around windows of at least --window seconds of back-to-back calls, after three warm-up calls; min and
median over --rounds windows.  Bytes per crop come from the shapes: the crop box read once (its mean area under the policy), the view
written and re-read once per pass over the workspace planes, the fp32 result written once -- what the kernel asks of the memory
system, most of it served by L2, not a measured traffic.  The share of a training step is against the committed dino_train_step
figure (81 ms for ViT-S/16 at 64 tiles).

For context only: the same chain written with Pillow calls on ONE CPU core of this host, records drawn on the device so that both
sides do the same work (--cpu-crops crops per view size)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DINO_STEP_MS = 81.0     # one dino_train_step of ViT-S/16 at 64 tiles


def crop_bytes(policy, h, w):
    """(read, workspace, written) bytes of one crop of `policy` from an h x w tile, from the shapes alone."""
    s = policy.size
    area = 0.5 * (policy.scale[0] + policy.scale[1]) * h * w
    passes = 1.0                                            # the resized view is written once ...
    passes += 3.75 * policy.p_jitter                        # ... read (and in 3 of 4 orders written) before contrast, read + written after,
    passes += 4.0 * policy.p_blur                           # read + written by each blur direction (its 3 box passes stay in LDS),
    passes += 1.0                                           # and read by the normalising pass
    return 3.0 * area, 3.0 * s * s * passes, 12.0 * s * s


def pil_chain(img, rec, size):
    """The reference's transform for one crop, written with Pillow calls (uint8 in, normalised float32 out)."""
    from PIL import Image, ImageEnhance, ImageFilter, ImageOps
    from snuffy_amd import augment
    x = Image.fromarray(img).crop((int(rec["left"]), int(rec["top"]), int(rec["left"] + rec["cw"]), int(rec["top"] + rec["ch"])))
    x = x.resize((size, size), Image.BICUBIC)
    if rec["flip"]:
        x = x.transpose(Image.FLIP_LEFT_RIGHT)
    if rec["jitter"]:
        for k in range(4):
            op = augment.OPS[(int(rec["order"]) >> (2 * k)) & 3]
            f = float(rec[op])
            if op == "brightness":
                x = ImageEnhance.Brightness(x).enhance(f)
            elif op == "contrast":
                x = ImageEnhance.Contrast(x).enhance(f)
            elif op == "saturation":
                x = ImageEnhance.Color(x).enhance(f)
            else:
                h, s, v = x.convert("HSV").split()
                nh = ((np.asarray(h).astype(np.int64) + int(f * 255)) % 256).astype(np.uint8)
                x = Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB")
    if rec["gray"]:
        l = x.convert("L")
        x = Image.merge("RGB", (l, l, l))
    if rec["blur"] > 0:
        x = x.filter(ImageFilter.GaussianBlur(radius=float(rec["blur"])))
    if rec["solarize"]:
        x = ImageOps.solarize(x, 128)
    t = np.asarray(x).astype(np.float32) / np.float32(255.0)
    return ((t - np.array(augment.IMAGENET_MEAN, np.float32)) / np.array(augment.IMAGENET_STD, np.float32)).transpose(2, 0, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cpu-crops", type=int, default=40)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    from snuffy_amd import augment, ops
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
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        n, total = 8, 0.0
        while True:                                         # grow the call count until one event pair spans the window
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            e1.synchronize()
            total = e0.elapsed_time(e1) * 1e-3
            if total >= args.window:
                return 1e3 * total / n
            n = max(n * 2, int(n * 1.2 * args.window / max(total, 1e-6)))

    g = torch.Generator().manual_seed(3)
    say("%s; device events around windows of >= %.1f s after 3 warm-up calls; min / median of %d windows"
        % (torch.cuda.get_device_name(0), args.window, args.rounds))
    say("%-34s %8s %20s %12s %28s %14s" % ("policy, tiles of 256 x 256", "crops", "ms per batch", "crops / s", "KB per crop (read+ws+out)",
                                          "of 81 ms step"))
    for name, make, b in (("DINO 2 x 224 + 8 x 96", lambda: augment.DINOAugment(seed=1), 64),
                          ("DINO 2 x 224 + 8 x 96", lambda: augment.DINOAugment(seed=1), 512),
                          ("MAE 1 x 224", lambda: augment.MAEAugment(seed=1), 64)):
        tiles = torch.randint(0, 256, (b, 256, 256, 3), dtype=torch.uint8, generator=g).to(dev)
        aug = make()
        crops = b * len(aug.policies)
        ms = sorted(window(lambda: aug(tiles)) for _ in range(args.rounds))
        parts = [crop_bytes(p, 256, 256) for p in aug.policies]
        kb = [sum(p[i] for p in parts) / len(parts) / 1024.0 for i in range(3)]
        share = "%.1f %%" % (100.0 * ms[len(ms) // 2] / DINO_STEP_MS) if (name.startswith("DINO") and b == 64) else "not measured"
        say("%-34s %8d %9.3f /%9.3f %12.0f %9.0f +%6.0f +%6.0f %14s" % ("%s, %d tiles" % (name, b), crops, ms[0], ms[len(ms) // 2],
                                                                        crops / (ms[len(ms) // 2] * 1e-3), kb[0], kb[1], kb[2], share))
        del tiles
    say("(share of the step: only the 64-tile DINO batch has a committed step time; the 512-tile step and the MAE step: not measured)")

    # context: the same records through Pillow on one CPU core
    torch.set_num_threads(1)
    policies = augment.dino_policies()
    tiles_np = np.random.default_rng(0).integers(0, 256, (args.cpu_crops, 256, 256, 3), dtype=np.uint8)
    table = augment.draw_params(policies, args.cpu_crops, 256, 256, ops.DeviceSampler(dev, seed=1, offset=0)).cpu().numpy()
    table = table.view(augment.RECORD_DTYPE).reshape(len(policies), args.cpu_crops)
    say("")
    say("context, not a comparison of like with like: the same chain in Pillow %s on one CPU core of this host, %d crops per view" %
        (__import__("PIL").__version__, args.cpu_crops))
    per_tile = 0.0
    for label, v in (("global view 1 (224, blur always)", 0), ("global view 2 (224, blur 0.1, solarise 0.2)", 1), ("local view (96, blur 0.5)", 2)):
        t0 = time.perf_counter()
        for i in range(args.cpu_crops):
            pil_chain(tiles_np[i], table[v, i], policies[v].size)
        ms = 1e3 * (time.perf_counter() - t0) / args.cpu_crops
        per_tile += ms * (8 if v == 2 else 1)
        say("  %-46s %7.2f ms per crop" % (label, ms))
    say("  one tile's 10 crops: %.1f ms on one core = %.0f tiles / s per core" % (per_tile, 1e3 / per_tile))
    return 0


if __name__ == "__main__":
    sys.exit(main())
