"""What the differentiable MFMA self-attention (ssl_pretrain.ViTAttentionFn: csrc/vit.hip forward with lse, csrc/vit_attn_bwd.hip
backward) buys adapter pre-training, against the parent's path -- the composition of torch ops under autograd (ssl_pretrain.FUSED_ATTENTION off).

    python tools/vit_attn_train_time.py [--rounds 3] [--window 0.5] [--out profiles/vit_attn_train.txt] [--only errors|attention|dino|mae]

  errors      lse and dQ / dK / dV of both arithmetics against float64 autograd over the table of tests/test_gpu_vit_attn_train.py, the torch
              composition of the same dtype beside them (the figures that test bounds)
  attention   forward + backward of ssl_pretrain._attention (qkv Linear, attention, proj Linear; fp32) at the recipes' shapes:
              DINO ViT-S/16 global views B = 128, T = 197, h = 6; local views B = 512, T = 37, h = 6; MAE ViT-B/16 encoder at 75 % masking
              B = 64, T = 50, h = 12
  dino        one dino_train_step of ViT-S/16 + adapters at 64 tiles (2 x 224^2 + 8 x 96^2), adapter tuning (trunk frozen)
  mae         one mae_train_step of the ViT-B/16 MAE-adapter model at batch 64, adapters training (trunk frozen)

One process; switch off and on alternate round by round; every leg is warmed, then timed with device events over a window of at least
--window seconds; the spread is min / median / max of the rounds.  A row is BEHIND when the medians' ratio is under 1 and the ranges do
not overlap, LEVEL when they do.  Peak memory: torch.cuda.max_memory_allocated over one step after a warm step.

    python tools/vit_attn_train_time.py --long [--out profiles/vit_attn_long_train.txt] [--only errors|attention|dino]

  the same method for 256 < T <= 4096 (csrc/vit_attn_bwd_long.hip; the switch is ssl_pretrain.FUSED_ATTENTION_LONG, FUSED_ATTENTION stays on):
  errors      dQ / dK / dV over the table of tests/test_gpu_vit_attn_long.py
  attention   forward + backward of _attention at ViT-S/8 global views B = 32, T = 785, h = 6, in fp32 and under bf16 autocast
  dino        one dino_train_step of ViT-S/8 + adapters at 64 tiles (2 x 224^2 at T = 785 + 8 x 96^2 at T = 145)

    python tools/vit_attn_train_time.py --dk32 [--out profiles/vit_attn_dk32_train.txt] [--only errors|attention|mae]

  the same method for heads 32 wide (csrc/vit_attn_dk32.hip; the switch is ssl_pretrain.FUSED_ATTENTION_DK32, the other two stay on):
  errors      out, lse and dQ / dK / dV over the table of tests/test_gpu_vit_attn_dk32.py
  attention   forward + backward of _attention at the MAE decoder's shape B = 64, T = 197, h = 16, D = 512, in fp32 and under bf16 autocast
  mae         the mae_train_step above (its eight decoder blocks are what the switch moves)"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TABLE = [(1, 1, 1), (2, 17, 1), (2, 32, 2), (2, 33, 1), (2, 37, 2), (3, 50, 3), (2, 197, 6), (2, 224, 2), (2, 225, 2), (2, 256, 2)]
FWD_ONLY = [(2, 785, 2), (1, 257, 2)]
LONG_TABLE = [(2, 257, 1), (1, 288, 2), (1, 511, 1), (2, 512, 1), (1, 513, 2), (2, 785, 2), (1, 1030, 1), (1, 2049, 1)]
DK32_TABLE = [(1, 1, 1), (2, 17, 1), (2, 32, 2), (2, 33, 3), (2, 37, 2), (3, 50, 3), (1, 100, 2), (1, 197, 16), (2, 224, 2), (2, 225, 2), (2, 256, 2)]


def composition(qkv, b, t, h):
    d = qkv.shape[1] // 3
    q, k, v = qkv.view(b, t, 3, h, d // h).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-2, -1)) * (d // h) ** -0.5
    return (s.softmax(-1) @ v).transpose(1, 2).reshape(b * t, d), s


def errors(say, dev, long_=False):
    import torch
    from snuffy_amd import ops
    from tests.helpers import rel_err

    def rel(a, b):
        return rel_err(a.cpu(), b.cpu()) if long_ else float((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-30))

    say("kernels against float64 autograd on the same operands (bf16 form: operands rounded to bf16 first); rel = %s;"
        % ("tests.helpers.rel_err" if long_ else "max |a - b| / max |b|"))
    say("'torch' = the composition of torch ops in the form's dtype on the device")
    say("%-6s %-14s %10s | %10s %10s %10s | %10s %10s %10s" % ("form", "(b, t, h)", "lse abs", "dQ rel", "dK rel", "dV rel", "torch dQ", "torch dK", "torch dV"))
    worst = {}
    for form in ("x3", "bf16"):
        for b, t, h in (LONG_TABLE if long_ else TABLE + FWD_ONLY):
            g = torch.Generator().manual_seed(1000 * t + 10 * h + b)
            qkv = torch.randn(b * t, 3 * h * 64, generator=g) * 1.5
            dout = torch.randn(b * t, h * 64, generator=g)
            if form == "bf16":
                qkv, dout = qkv.bfloat16(), dout.bfloat16()
            q64 = qkv.to(dev).double().requires_grad_(True)
            out, s = composition(q64, b, t, h)
            out.backward(dout.to(dev).double())
            qd, dd = qkv.to(dev), dout.to(dev)
            _, lse = ops.vit_attention_fwd_lse(qd, b, t, h)
            e_lse = float((lse.double() - torch.logsumexp(s.detach(), -1)).abs().max())
            worst[(form, "lse")] = max(worst.get((form, "lse"), 0.0), e_lse)
            if not long_ and (b, t, h) in FWD_ONLY:
                say("%-6s %-14s %10.3g | (forward only: above the backward's T)" % (form, (b, t, h), e_lse))
                continue
            dqkv = (ops.vit_attention_bwd_long if long_ else ops.vit_attention_bwd)(qd, dd, lse, b, t, h)
            qc = qd.clone().requires_grad_(True)
            composition(qc, b, t, h)[0].backward(dd)
            d = h * 64
            cols = []
            for got in (dqkv, qc.grad):
                for lo in (0, d, 2 * d):
                    want = q64.grad[:, lo:lo + d]
                    cols.append(rel(got[:, lo:lo + d], want) if float(want.abs().max()) > 0 else float(got[:, lo:lo + d].abs().max()))
            worst[(form, "bwd")] = max([worst.get((form, "bwd"), 0.0)] + cols[:3])
            say("%-6s %-14s %10.3g | %10.3g %10.3g %10.3g | %10.3g %10.3g %10.3g" % ((form, (b, t, h), e_lse) + tuple(cols)))
    for form in ("x3", "bf16"):
        say("largest over the table, %s: lse %.3g, backward %.3g" % (form, worst[(form, "lse")], worst[(form, "bwd")]))


def errors_dk32(say, dev):
    import torch
    from snuffy_amd import ops
    from tests.helpers import rel_err

    say("kernels against float64 autograd of the composition on the same operands, computed on the CPU (bf16 form: operands rounded to bf16")
    say("first); rel = tests.helpers.rel_err; 'torch' = the composition of torch ops in the form's dtype on the device")
    say("%-6s %-14s %10s %10s %10s | %10s %10s %10s | %10s %10s %10s" % ("form", "(b, t, h)", "lse abs", "out rel", "torch out", "dQ rel", "dK rel",
                                                                      "dV rel", "torch dQ", "torch dK", "torch dV"))
    worst = {}

    def note(form, what, v):
        worst[(form, what)] = max(worst.get((form, what), 0.0), v)

    for form in ("x3", "bf16"):
        for b, t, h in DK32_TABLE:
            g = torch.Generator().manual_seed(1000 * t + 10 * h + b)
            qkv = torch.randn(b * t, 3 * h * 32, generator=g) * 1.5
            dout = torch.randn(b * t, h * 32, generator=g)
            if form == "bf16":
                qkv, dout = qkv.bfloat16(), dout.bfloat16()
            q64 = qkv.double().requires_grad_(True)
            out64, s = composition(q64, b, t, h)
            out64.backward(dout.double())
            qd, dd = qkv.to(dev), dout.to(dev)
            out, lse = ops.vit_attention_dk32_fwd_lse(qd, b, t, h)
            dqkv = ops.vit_attention_dk32_bwd(qd, dd, lse, b, t, h)
            qc = qd.clone().requires_grad_(True)
            oc = composition(qc, b, t, h)[0]
            oc.backward(dd)
            e_lse = float((lse.cpu().double() - torch.logsumexp(s.detach(), -1)).abs().max())
            e_out, e_outc = rel_err(out.cpu(), out64.detach()), rel_err(oc.detach().cpu(), out64.detach())
            d = h * 32
            cols = []
            for got in (dqkv.cpu(), qc.grad.cpu()):
                for lo in (0, d, 2 * d):
                    want = q64.grad[:, lo:lo + d]
                    cols.append(rel_err(got[:, lo:lo + d], want) if float(want.abs().max()) > 0 else float(got[:, lo:lo + d].abs().max()))
            note(form, "lse", e_lse), note(form, "out", e_out), note(form, "torch out", e_outc), note(form, "bwd", max(cols[:3]))
            say("%-6s %-14s %10.3g %10.3g %10.3g | %10.3g %10.3g %10.3g | %10.3g %10.3g %10.3g" % ((form, (b, t, h), e_lse, e_out, e_outc) + tuple(cols)))
    for form in ("x3", "bf16"):
        say("largest over the table, %s: lse %.3g, out %.3g (torch composition %.3g), backward %.3g"
            % (form, worst[(form, "lse")], worst[(form, "out")], worst[(form, "torch out")], worst[(form, "bwd")]))
    say("gates of tests/test_gpu_vit_attn_dk32.py (4 x the largest for the fp32 class, 2 x for bf16, one digit up; out: of the larger of kernel")
    say("and torch composition): lse x3 1e-4 (the cap: 4 x 5.1e-5 is above it; the figure is the x3 scores' own error, the 64-wide pair has")
    say("5.2e-5), bf16 3e-6 (cap 5e-2); backward x3 2e-4 (the cap), bf16 2e-2 (cap 3e-2); out x3 7e-5, bf16 4e-2")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out")
    ap.add_argument("--only", help="'errors', 'attention', 'dino' or 'mae'")
    ap.add_argument("--long", action="store_true", help="the shapes above 256 tokens and the switch FUSED_ATTENTION_LONG")
    ap.add_argument("--dk32", action="store_true", help="heads 32 wide (the MAE decoder) and the switch FUSED_ATTENTION_DK32")
    args = ap.parse_args()
    if args.long and args.dk32:
        ap.error("--long and --dk32 are separate modes")
    import torch
    from snuffy_amd import ssl_pretrain as S
    from snuffy_amd import vit
    if not torch.cuda.is_available():
        print("no GPU: nothing measured")
        return 1
    dev = torch.device("cuda:0")
    lines = []
    switch = "FUSED_ATTENTION_LONG" if args.long else ("FUSED_ATTENTION_DK32" if args.dk32 else "FUSED_ATTENTION")

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
                setattr(S, switch, on)
                torch.manual_seed(5)
                t[on].append(window(fn))
        return sorted(t[False]), sorted(t[True])

    def peaks(fn):
        peak = {}
        for on in (False, True):
            setattr(S, switch, on)
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

    def row(tag, fn, with_peak):
        peak = peaks(fn) if with_peak else None
        off, on_ = alternate(fn)
        sp = off[len(off) // 2] / on_[len(on_) // 2]
        behind = sp < 1.0 and on_[0] > off[-1]
        if behind:
            behind_rows.append(tag)
        note = "   BEHIND" if behind else ("" if sp >= 1.0 else "   (level: ranges overlap)")
        say("%-44s %s %s %7.2fx%s%s" % (tag, fmt(off), fmt(on_), sp, ("  %8.0f -> %-7.0f" % (peak[False], peak[True])) if peak else "", note))

    shipped = getattr(S, switch)
    say("adapter pre-training, self-attention on the MFMA kernels (on) against the autograd composition (off); %s; %s"
        % ("T > 256, switch FUSED_ATTENTION_LONG" if args.long else ("dk = 32, switch FUSED_ATTENTION_DK32" if args.dk32 else "fp32"),
           torch.cuda.get_device_name(0)))
    if not args.only or args.only == "errors":
        say("")
        errors_dk32(say, dev) if args.dk32 else errors(say, dev, args.long)
    head = "%-44s %29s %29s %8s" % ("ms (min / median / max of %d alternating rounds)" % args.rounds, "off  min    median       max",
                                    "on   min    median       max", "speedup")
    if args.long and (not args.only or args.only == "attention"):
        say("")
        say("forward + backward of ssl_pretrain._attention (qkv Linear, attention, proj Linear), gradient to the input")
        say(head + "  peak MB off -> on")
        for tag, cast in (("DINO ViT-S/8 global B=32 T=785 h=6 fp32", False), ("DINO ViT-S/8 global B=32 T=785 h=6 autocast bf16", True)):
            torch.manual_seed(1)
            attn = vit.Attention(384, num_heads=6, qkv_bias=True).to(dev)
            x = torch.randn(32, 785, 384, device=dev, requires_grad=True)
            dy = torch.randn(32, 785, 384, device=dev)

            def one():
                x.grad = None
                with torch.autocast("cuda", torch.bfloat16, enabled=cast):
                    y = S._attention(attn, x)
                y.backward(dy.to(y.dtype))

            row(tag, one, True)
            del attn, x, dy
    if args.long and (not args.only or args.only == "dino"):
        say("")
        say("one dino_train_step: ViT-S/8 + adapters (adapter tuning), 64 tiles as 2 x 224^2 (T = 785) + 8 x 96^2 (T = 145, the short kernels "
            "in both legs) crops, out_dim 65536")
        say(head + "  peak MB off -> on")
        torch.manual_seed(2)

        def net8():
            bb = vit.vit_small(8, adapter_ffn_layernorm_option="none", adapter_ffn_init_option="lora", adapter_ffn_scalar="0.1",
                               adapter_ffn_num=64, adapter_d_model=384)
            return S.MultiCropWrapper(bb, S.DINOHead(384, 65536)).to(dev).train()

        student, teacher = net8(), net8()
        teacher.load_state_dict(student.state_dict())
        for p in teacher.parameters():
            p.requires_grad = False
        S.freeze_for_adapter_tuning(student)
        loss_mod = S.DINOLoss(65536, 10, 0.04, 0.04, 0, 10).to(dev)
        opt = torch.optim.AdamW(S.get_params_groups(student), lr=1e-5)
        crops = [torch.randn(64, 3, 224, 224, device=dev) for _ in range(2)] + [torch.randn(64, 3, 96, 96, device=dev) for _ in range(8)]
        row("dino_train_step ViT-S/8 64 tiles", lambda: S.dino_train_step(student, teacher, loss_mod, crops, opt, 1, clip_grad=3.0), True)
        del student, teacher, loss_mod, opt, crops
        torch.cuda.empty_cache()
    if args.dk32 and (not args.only or args.only == "attention"):
        say("")
        say("forward + backward of ssl_pretrain._attention (qkv Linear, attention, proj Linear), gradient to the input")
        say(head + "  peak MB off -> on")
        for tag, cast in (("MAE decoder B=64 T=197 h=16 D=512 fp32", False), ("MAE decoder B=64 T=197 h=16 D=512 autocast bf16", True)):
            torch.manual_seed(1)
            attn = vit.Attention(512, num_heads=16, qkv_bias=True).to(dev)
            x = torch.randn(64, 197, 512, device=dev, requires_grad=True)
            dy = torch.randn(64, 197, 512, device=dev)

            def one():
                x.grad = None
                with torch.autocast("cuda", torch.bfloat16, enabled=cast):
                    y = S._attention(attn, x)
                y.backward(dy.to(y.dtype))

            row(tag, one, True)
            del attn, x, dy
    if not args.long and not args.dk32 and (not args.only or args.only == "attention"):
        say("")
        say("forward + backward of ssl_pretrain._attention (qkv Linear, attention, proj Linear), gradient to the input")
        say(head)
        for tag, b, t, d, h in (("DINO ViT-S/16 global B=128 T=197 h=6", 128, 197, 384, 6), ("DINO ViT-S/16 local  B=512 T=37  h=6", 512, 37, 384, 6),
                                ("MAE  ViT-B/16 enc 75% B=64  T=50  h=12", 64, 50, 768, 12)):
            torch.manual_seed(1)
            attn = vit.Attention(d, num_heads=h, qkv_bias=True).to(dev)
            x = torch.randn(b, t, d, device=dev, requires_grad=True)
            dy = torch.randn(b, t, d, device=dev)

            def one():
                x.grad = None
                S._attention(attn, x).backward(dy)

            row(tag, one, False)
            del attn, x, dy
    if not args.long and not args.dk32 and (not args.only or args.only == "dino"):
        say("")
        say("one dino_train_step: ViT-S/16 + adapters (adapter tuning), 64 tiles as 2 x 224^2 + 8 x 96^2 crops, out_dim 65536; peak MB off -> on")
        say(head + "  peak MB off -> on")
        torch.manual_seed(2)

        def net():
            bb = vit.vit_small(16, adapter_ffn_layernorm_option="none", adapter_ffn_init_option="lora", adapter_ffn_scalar="0.1",
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
        row("dino_train_step 64 tiles", lambda: S.dino_train_step(student, teacher, loss_mod, crops, opt, 1, clip_grad=3.0), True)
        del student, teacher, loss_mod, opt, crops
        torch.cuda.empty_cache()
    if not args.long and (not args.only or args.only == "mae"):
        say("")
        say("one mae_train_step: ViT-B/16 MAE-adapter model (decoder 512 x 8, 16 heads: dk = 32, T = 197; %s), batch 64, mask 0.75"
            % ("the switch moves these eight blocks, the encoder's twelve run the 64-wide kernels in both legs" if args.dk32 else
               "the decoder follows FUSED_ATTENTION_DK32 in both legs, shipped %s" % ("on" if S.FUSED_ATTENTION_DK32 else "off")))
        say(head + "  peak MB off -> on")
        torch.manual_seed(3)
        model = S.MAEPretrainModel(img_size=224, patch_size=16, embed_dim=768, depth=12, num_heads=12, decoder_embed_dim=512, decoder_depth=8,
                                   decoder_num_heads=16, norm_pix_loss=True, adapter_ffn_num=64, adapter_d_model=768).to(dev).train()
        for n, p in model.named_parameters():
            p.requires_grad = "adaptmlp" in n
        opt = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=1e-5, betas=(0.9, 0.95))
        imgs = torch.randn(64, 3, 224, 224, device=dev)
        row("mae_train_step batch 64", lambda: S.mae_train_step(model, imgs, opt), True)
        del model, opt, imgs
    setattr(S, switch, shipped)
    if not args.only:
        say("")
        say("ship rule (on only if no step row is behind outside the spread): the timing lets %s ship %s%s"
            % (switch, "OFF" if behind_rows else "ON", (" -- behind at " + ", ".join(behind_rows)) if behind_rows else ""))
    return 0


if __name__ == "__main__":
    sys.exit(main())
