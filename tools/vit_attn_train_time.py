"""What the differentiable MFMA self-attention (ssl_pretrain.ViTAttentionFn: csrc/vit.hip forward with lse, csrc/vit_attn_bwd.hip
backward) buys adapter pre-training, against the parent's path -- the composition of torch ops under autograd (ssl_pretrain.FUSED_ATTENTION off).

    python tools/vit_attn_train_time.py [--rounds 3] [--window 0.5] [--out profiles/vit_attn_train.txt] [--only errors|attention|dino|mae]

  errors      lse and dQ / dK / dV of both arithmetics against float64 autograd over the `short` row of tests/vit_attn_forms.py, the torch
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
  errors      dQ / dK / dV over the `long` row of tests/vit_attn_forms.py
  attention   forward + backward of _attention at ViT-S/8 global views B = 32, T = 785, h = 6, in fp32 and under bf16 autocast
  dino        one dino_train_step of ViT-S/8 + adapters at 64 tiles (2 x 224^2 at T = 785 + 8 x 96^2 at T = 145)

    python tools/vit_attn_train_time.py --dk32 [--out profiles/vit_attn_dk32_train.txt] [--only errors|attention|mae]

  the same method for heads 32 wide (csrc/vit_attn_dk32.hip; the switch is ssl_pretrain.FUSED_ATTENTION_DK32, the other two stay on):
  errors      out, lse and dQ / dK / dV over the `dk32` row of tests/vit_attn_forms.py
  attention   forward + backward of _attention at the MAE decoder's shape B = 64, T = 197, h = 16, D = 512, in fp32 and under bf16 autocast
  mae         the mae_train_step above (its eight decoder blocks are what the switch moves)

The three modes are one record each (`modes`): the form's row of tests/vit_attn_forms.py -- shape tables, ops names and switch are read
from there, not repeated here -- and what the error table and the timed sections differ in.  The printed text is that of the committed
profiles/vit_attn_*_train.txt, which this tool reproduces."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _max_ratio(a, b):
    return float((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _rel_err(a, b):
    from tests.helpers import rel_err
    return rel_err(a.cpu(), b.cpu())


def modes():
    """One record per mode of the command line: the form's row of tests/vit_attn_forms.py (shape tables, ops names, switch), what the
    error table measures with and where its float64 reference is computed, whether it has the `out` columns, the text around it, and
    the rows of the attention and step sections: (tag, B, T, D, h, autocast, peak memory)."""
    from tests import vit_attn_forms as V
    same_operands = ["kernels against float64 autograd on the same operands (bf16 form: operands rounded to bf16 first); rel = %s;",
                     "'torch' = the composition of torch ops in the form's dtype on the device"]
    return {
        None: V._row(row=V.SHORT, title="fp32", rel=_max_ratio, ref_on_device=True, out_cols=False,
                     head=[same_operands[0] % "max |a - b| / max |b|", same_operands[1]], tail=[],
                     attention=[("DINO ViT-S/16 global B=128 T=197 h=6", 128, 197, 384, 6, False, False),
                                ("DINO ViT-S/16 local  B=512 T=37  h=6", 512, 37, 384, 6, False, False),
                                ("MAE  ViT-B/16 enc 75% B=64  T=50  h=12", 64, 50, 768, 12, False, False)],
                     dino=(16, "one dino_train_step: ViT-S/16 + adapters (adapter tuning), 64 tiles as 2 x 224^2 + 8 x 96^2 crops, out_dim 65536; "
                               "peak MB off -> on", "dino_train_step 64 tiles"), mae=True),
        "long": V._row(row=V.LONG, title="T > 256, switch FUSED_ATTENTION_LONG", rel=_rel_err, ref_on_device=True, out_cols=False,
                       head=[same_operands[0] % "tests.helpers.rel_err", same_operands[1]], tail=[],
                       attention=[("DINO ViT-S/8 global B=32 T=785 h=6 fp32", 32, 785, 384, 6, False, True),
                                  ("DINO ViT-S/8 global B=32 T=785 h=6 autocast bf16", 32, 785, 384, 6, True, True)],
                       dino=(8, "one dino_train_step: ViT-S/8 + adapters (adapter tuning), 64 tiles as 2 x 224^2 (T = 785) + 8 x 96^2 (T = 145, the "
                                "short kernels in both legs) crops, out_dim 65536", "dino_train_step ViT-S/8 64 tiles"), mae=False),
        "dk32": V._row(row=V.DK32, title="dk = 32, switch FUSED_ATTENTION_DK32", rel=_rel_err, ref_on_device=False, out_cols=True,
                       head=["kernels against float64 autograd of the composition on the same operands, computed on the CPU (bf16 form: operands "
                             "rounded to bf16", "first); rel = tests.helpers.rel_err; 'torch' = the composition of torch ops in the form's dtype on "
                             "the device"],
                       tail=["gates of tests/test_gpu_vit_attn_dk32.py (4 x the largest for the fp32 class, 2 x for bf16, one digit up; out: of the larger of "
                             "kernel", "and torch composition): lse x3 1e-4 (the cap: 4 x 5.1e-5 is above it; the figure is the x3 scores' own error, "
                             "the 64-wide pair has", "5.2e-5), bf16 3e-6 (cap 5e-2); backward x3 2e-4 (the cap), bf16 2e-2 (cap 3e-2); out x3 7e-5, "
                             "bf16 4e-2"],
                       attention=[("MAE decoder B=64 T=197 h=16 D=512 fp32", 64, 197, 512, 16, False, True),
                                  ("MAE decoder B=64 T=197 h=16 D=512 autocast bf16", 64, 197, 512, 16, True, True)],
                       dino=None, mae=True),
    }


def errors(say, dev, mode):
    import torch
    from snuffy_amd import ops
    from tests import vit_attn_forms as V

    row, rel = mode.row, mode.rel
    fwd, bwd = getattr(ops, row.fwd), getattr(ops, row.bwd)
    ref = dev if mode.ref_on_device else "cpu"
    for line in mode.head:
        say(line)
    outs = ("out rel", "torch out") if mode.out_cols else ()
    say(("%-6s %-14s" + " %10s" * (1 + len(outs)) + " | %10s %10s %10s | %10s %10s %10s")
        % (("form", "(b, t, h)", "lse abs") + outs + ("dQ rel", "dK rel", "dV rel", "torch dQ", "torch dK", "torch dV")))
    worst = {}

    def note(form, what, v):
        worst[(form, what)] = max(worst.get((form, what), 0.0), v)

    for form in V.ARITHMETICS:
        for b, t, h in row.shapes + row.fwd_only:
            qkv, dout = V.operands(row.dk, form, b, t, h)
            q64 = qkv.to(ref).double().requires_grad_(True)
            out64, s = V.composition(q64, b, t, h)
            out64.backward(dout.to(ref).double())
            qd, dd = qkv.to(dev), dout.to(dev)
            out, lse = fwd(qd, b, t, h)
            e_lse = float((lse.to(ref).double() - torch.logsumexp(s.detach(), -1)).abs().max())
            note(form, "lse", e_lse)
            if (b, t, h) in row.fwd_only:
                say("%-6s %-14s %10.3g | (forward only: above the backward's T)" % (form, (b, t, h), e_lse))
                continue
            dqkv = bwd(qd, dd, lse, b, t, h)
            qc = qd.clone().requires_grad_(True)
            oc = V.composition(qc, b, t, h)[0]
            oc.backward(dd)
            e_outs = (rel(out, out64.detach()), rel(oc.detach(), out64.detach())) if mode.out_cols else ()
            d = h * row.dk
            cols = []
            for got in (dqkv.to(ref), qc.grad.to(ref)):
                for lo in (0, d, 2 * d):
                    want = q64.grad[:, lo:lo + d]
                    cols.append(rel(got[:, lo:lo + d], want) if float(want.abs().max()) > 0 else float(got[:, lo:lo + d].abs().max()))
            for what, v in zip(("out", "torch out"), e_outs):
                note(form, what, v)
            note(form, "bwd", max(cols[:3]))
            say(("%-6s %-14s" + " %10.3g" * (1 + len(e_outs)) + " | %10.3g %10.3g %10.3g | %10.3g %10.3g %10.3g")
                % ((form, (b, t, h), e_lse) + e_outs + tuple(cols)))
    for form in V.ARITHMETICS:
        say("largest over the table, %s: lse %.3g, %sbackward %.3g"
            % (form, worst[(form, "lse")], ("out %.3g (torch composition %.3g), " % (worst[(form, "out")], worst[(form, "torch out")]))
               if mode.out_cols else "", worst[(form, "bwd")]))
    for line in mode.tail:
        say(line)


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
    mode = modes()["long" if args.long else ("dk32" if args.dk32 else None)]
    switch = mode.row.switch

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
        % (mode.title, torch.cuda.get_device_name(0)))
    if not args.only or args.only == "errors":
        say("")
        errors(say, dev, mode)
    head = "%-44s %29s %29s %8s" % ("ms (min / median / max of %d alternating rounds)" % args.rounds, "off  min    median       max",
                                    "on   min    median       max", "speedup")
    if not args.only or args.only == "attention":
        say("")
        say("forward + backward of ssl_pretrain._attention (qkv Linear, attention, proj Linear), gradient to the input")
        say(head + ("  peak MB off -> on" if any(r[-1] for r in mode.attention) else ""))
        for tag, b, t, d, h, cast, with_peak in mode.attention:
            torch.manual_seed(1)
            attn = vit.Attention(d, num_heads=h, qkv_bias=True).to(dev)
            x = torch.randn(b, t, d, device=dev, requires_grad=True)
            dy = torch.randn(b, t, d, device=dev)

            def one():
                x.grad = None
                if cast:
                    with torch.autocast("cuda", torch.bfloat16):
                        y = S._attention(attn, x)
                else:
                    y = S._attention(attn, x)
                y.backward(dy.to(y.dtype))

            row(tag, one, with_peak)
            del attn, x, dy
    if mode.dino and (not args.only or args.only == "dino"):
        patch, text, tag = mode.dino
        say("")
        say(text)
        say(head + "  peak MB off -> on")
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
        row(tag, lambda: S.dino_train_step(student, teacher, loss_mod, crops, opt, 1, clip_grad=3.0), True)
        del student, teacher, loss_mod, opt, crops
        torch.cuda.empty_cache()
    if mode.mae and (not args.only or args.only == "mae"):
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
