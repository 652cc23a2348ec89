"""What the frozen-trunk training route (ssl_pretrain.FUSED_TRUNK: frozen Linear / LayerNorm / GELU of every block on the fp32-class MFMA
GEMMs and the row kernels of csrc/vit_train.hip) buys adapter pre-training in fp32, against the switch-off leg -- the torch ops of the parent
(tests/test_gpu_vit_trunk_train.py shows that leg to be bit-identical to the parent's path).

    python tools/vit_trunk_train_time.py [--rounds 3] [--window 0.5] [--out profiles/vit_trunk_train.txt] [--only errors|blocks|dino|dino8|mae]

  errors   the two row kernels in both image formats against float64 over tests/vit_trunk_forms.KERNEL_SHAPES (the figures the gates
           of that file are chosen from)
  blocks   one frozen block, switch on against off and each against a float64 composition (BLOCK_SHAPES and the hl case)
  dino     one dino_train_step of ViT-S/16 + adapters at 64 tiles (2 x 224^2 + 8 x 96^2), adapter tuning (trunk frozen)
  dino8    the same of ViT-S/8
  mae      one mae_train_step of the ViT-B/16 MAE-adapter model at batch 64, adapters training (trunk frozen)

One process; switch off and on alternate round by round; every leg is warmed, then timed with device events over a window of at least
--window seconds; the spread is min / median / max of the rounds.  A row is BEHIND when the medians' ratio is under 1 and the ranges do
not overlap, LEVEL when they do.  Peak memory: torch.cuda.max_memory_allocated over one step after a warm step.

    python tools/vit_trunk_train_time.py --step on|off [--steps 5]

  runs that many DINO ViT-S/16 steps with the switch forced, nothing else: the program a kernel trace is taken of
  (rocprofv3 --kernel-trace --stats -- python tools/vit_trunk_train_time.py --step on).

    python tools/vit_trunk_train_time.py --share <kernel stats csv> [--label on]

  the share of the traced kernel time spent in GEMM kernels (ours: names with gemm_; the library's: Cijk_ / Custom_Cijk_), from the
  kernel statistics such a trace writes."""
import argparse
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SWITCH = "FUSED_TRUNK"


def share(path, label):
    rows = list(csv.DictReader(open(path)))
    name = next(k for k in rows[0] if k.lower() in ("name", "kernelname", "kernel_name"))
    dur = next(k for k in rows[0] if k.lower() in ("totaldurationns", "total_duration_ns", "totalduration"))
    total = sum(float(r[dur]) for r in rows)
    kinds = {"our MFMA GEMMs": lambda n: "gemm_" in n and "Cijk" not in n, "library GEMMs": lambda n: "Cijk" in n,
             "attention kernels": lambda n: "vit_att" in n or "vit_bwd" in n or "attention" in n, "GELU row kernels": lambda n: "gelu_image" in n,
             "split / LayerNorm row kernels": lambda n: "split" in n or "layernorm" in n}
    print("kernel time by kind, switch %s (%d kernel names, %.1f ms traced):" % (label, len(rows), total / 1e6))
    for kind, pick in kinds.items():
        t = sum(float(r[dur]) for r in rows if pick(r[name]))
        print("   %-30s %8.1f ms  %5.1f %%" % (kind, t / 1e6, 100.0 * t / total))
    for r in sorted(rows, key=lambda r: -float(r[dur]))[:8]:
        print("   top: %6.1f %%  %s" % (100.0 * float(r[dur]) / total, r[name][:110]))
    return 0


def dino_step(S, vit, torch, dev, patch):
    torch.manual_seed(2)

    def net():
        bb = vit.vit_small(patch, adapter_ffn_layernorm_option="none", adapter_ffn_init_option="lora", adapter_ffn_scalar="0.1",
                           adapter_ffn_num=64, adapter_d_model=384)
        return S.MultiCropWrapper(bb, S.DINOHead(384, 65536)).to(dev).train()

    student, teacher = net(), net()
    teacher.load_state_dict(student.state_dict())
    for p in teacher.parameters():
        p.requires_grad = False
    S.freeze_for_adapter_tuning(student)
    loss_mod = S.DINOLoss(65536, 10, 0.04, 0.04, 0, 10).to(dev)
    opt = torch.optim.AdamW(S.get_params_groups(student), lr=1e-5)
    crops = [torch.randn(64, 3, 224, 224, device=dev) for _ in range(2)] + [torch.randn(64, 3, 96, 96, device=dev) for _ in range(8)]
    return lambda: S.dino_train_step(student, teacher, loss_mod, crops, opt, 1, clip_grad=3.0)


def mae_step(S, torch, dev):
    torch.manual_seed(3)
    model = S.MAEPretrainModel(img_size=224, patch_size=16, embed_dim=768, depth=12, num_heads=12, decoder_embed_dim=512, decoder_depth=8,
                               decoder_num_heads=16, norm_pix_loss=True, adapter_ffn_num=64, adapter_d_model=768).to(dev).train()
    for n, p in model.named_parameters():
        p.requires_grad = "adaptmlp" in n
    opt = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=1e-5, betas=(0.9, 0.95))
    imgs = torch.randn(64, 3, 224, 224, device=dev)
    return lambda: S.mae_train_step(model, imgs, opt)


def errors(say, ops):
    from tests import vit_trunk_forms as V
    say("row kernels of csrc/vit_train.hip: the decoded image (hi + lo) against float64 of the same fp32 operands, max |a - b| / max |b|;")
    say("operands: normal draws x 3 with 0, -0, +-1e-30, +-6, +-40 planted")
    say("%-22s %12s %12s %12s %12s" % ("(m, n)", "gelu hl", "gelu cat", "gelu_bwd hl", "gelu_bwd cat"))
    worst = {}
    for m, n, strided in V.KERNEL_SHAPES:
        e = V.kernel_errors(ops, m, n, strided)
        for k, v in e.items():
            worst[k[0]] = max(worst.get(k[0], 0.0), v)
        say("%-22s %12.3g %12.3g %12.3g %12.3g" % ("(%d, %d)%s" % (m, n, " row-strided" if strided else ""), e[("gelu", "hl")], e[("gelu", "cat")],
                                                  e[("gelu_bwd", "hl")], e[("gelu_bwd", "cat")]))
    say("largest over the table: gelu %.3g, gelu_bwd %.3g; cap 2^-15 = %.3g (16 significant bits of the split, one more for the fp32 erff)"
        % (worst["gelu"], worst["gelu_bwd"], V.KERNEL_CAP))
    say("gates of tests/vit_trunk_forms.py (4 x the largest, one digit up, never above the cap): gelu %.0e, gelu_bwd %.0e"
        % (V.GELU_GATE, V.GELU_BWD_GATE))


def blocks(say, ops, S):
    from tests import vit_trunk_forms as V
    say("one frozen block (adapters train, adapter dropout 0), forward + backward: switch on against off, and each against a float64")
    say("composition of the same block; max |a - b| / max |b|; the on / off gate of the tests is %.0e (a cap)" % V.ONOFF_GATE)
    say("%-24s %-18s %10s %10s %10s" % ("(B, T, D, h)", "tensor", "on / off", "on / f64", "off / f64"))
    t, d, h, bott = V.BLOCK_HL
    for b, t, d, h, bott in V.BLOCK_SHAPES + [(V.hl_batch(ops, t, d), t, d, h, bott)]:
        blk = V.frozen_block(d, h, bott)
        x0, dy = V.block_operands(b, t, d)
        res = {}
        for flag in (True, False):
            setattr(S, SWITCH, flag)
            res[flag] = V.run_block(S, blk, x0, dy)
        ref = V.block_float64(S, blk, x0, dy)
        for (name, on), (_, off), (_, want) in zip(res[True], res[False], ref):
            say("%-24s %-18s %10.3g %10.3g %10.3g" % ((b, t, d, h), name, V.rel_err(on, off), V.rel_err(on, want), V.rel_err(off, want)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out")
    ap.add_argument("--only", help="'errors', 'blocks', 'dino', 'dino8' or 'mae'")
    ap.add_argument("--step", choices=["on", "off"], help="run DINO ViT-S/16 steps with the switch forced and nothing else (for a kernel trace)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--share", help="kernel statistics csv of a trace: print the share of GEMM kernels")
    ap.add_argument("--label", default="?")
    args = ap.parse_args()
    if args.share:
        return share(args.share, args.label)
    import torch
    from snuffy_amd import ops, vit
    from snuffy_amd import ssl_pretrain as S
    if not torch.cuda.is_available():
        print("no GPU: nothing measured")
        return 1
    dev = torch.device("cuda:0")
    if args.step:
        setattr(S, SWITCH, args.step == "on")
        fn = dino_step(S, vit, torch, dev, 16)
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        return 0
    lines = []

    def say(s):
        lines.append(s + "\n")
        print(s, flush=True)
        if args.out:
            open(args.out, "w").writelines(lines)

    def window(fn):
        """ms per call: device events around batches of calls until --window seconds of device time have been covered."""
        fn()
        torch.cuda.synchronize()
        total, n, batch = 0.0, 0, 1
        while total < 1e3 * args.window or n < 2:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(batch):
                fn()
            e1.record()
            e1.synchronize()
            dt = e0.elapsed_time(e1)
            total, n = total + dt, n + batch
            batch = max(1, min(256, int(batch * 50.0 / max(dt, 1e-3))))      # batches of ~50 ms
        return total / n

    def alternate(fn):
        t = {False: [], True: []}
        for _ in range(args.rounds):
            for on in (False, True):
                setattr(S, SWITCH, on)
                torch.manual_seed(5)
                t[on].append(window(fn))
        return sorted(t[False]), sorted(t[True])

    def peaks(fn):
        peak = {}
        for on in (False, True):
            setattr(S, SWITCH, on)
            fn()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            fn()
            torch.cuda.synchronize()
            peak[on] = torch.cuda.max_memory_allocated() / 2 ** 20
        return peak

    def fmt(ts):
        return "%9.3f %9.3f %9.3f" % (ts[0], ts[len(ts) // 2], ts[-1])

    behind_rows = []

    def row(tag, fn):
        peak = peaks(fn)
        off, on_ = alternate(fn)
        sp = off[len(off) // 2] / on_[len(on_) // 2]
        behind = sp < 1.0 and on_[0] > off[-1]
        if behind:
            behind_rows.append(tag)
        note = "   BEHIND" if behind else ("" if sp >= 1.0 else "   (level: ranges overlap)")
        say("%-44s %s %s %7.2fx  %8.0f -> %-7.0f%s" % (tag, fmt(off), fmt(on_), sp, peak[False], peak[True], note))

    shipped = getattr(S, SWITCH)
    say("adapter pre-training in fp32, the frozen trunk on the fp32-class MFMA GEMMs (on) against the torch ops (off); one %s (%s)"
        % ("MI355X" if "gfx950" in torch.cuda.get_device_properties(0).gcnArchName else torch.cuda.get_device_name(0),
           torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]))
    if not args.only or args.only == "errors":
        say("")
        errors(say, ops)
    if not args.only or args.only == "blocks":
        say("")
        blocks(say, ops, S)
    head = "%-44s %29s %29s %8s  peak MB off -> on" % ("ms (min / median / max of %d alternating rounds)" % args.rounds,
                                                      "off  min    median       max", "on   min    median       max", "speedup")
    steps = (("dino", "dino_train_step ViT-S/16 64 tiles", lambda: dino_step(S, vit, torch, dev, 16)),
             ("dino8", "dino_train_step ViT-S/8 64 tiles", lambda: dino_step(S, vit, torch, dev, 8)),
             ("mae", "mae_train_step ViT-B/16 batch 64", lambda: mae_step(S, torch, dev)))
    if not args.only or args.only in [s[0] for s in steps]:
        say("")
        say("whole training steps, trunk frozen, adapters (and the DINO head) training: 2 x 224^2 + 8 x 96^2 crops of 64 tiles, out_dim 65536;")
        say("MAE-adapter model with decoder 512 x 8, mask 0.75; attention switches as shipped in both legs")
        say(head)
        for key, tag, make in steps:
            if not args.only or args.only == key:
                fn = make()
                row(tag, fn)
                del fn
                torch.cuda.empty_cache()
    setattr(S, SWITCH, shipped)
    if not args.only:
        say("")
        say("ship rule (on only if no step row is behind outside the spread): the timing lets %s ship %s%s"
            % (SWITCH, "OFF" if behind_rows else "ON", (" -- behind at " + ", ".join(behind_rows)) if behind_rows else ""))
    return 0


if __name__ == "__main__":
    sys.exit(main())
