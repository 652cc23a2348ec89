#!/usr/bin/env python3
"""What the fp32-class chains launch and compute, written down so that two versions of the package can be compared line by line.

  python tools/split_formats_trace.py --package DIR --out FILE.json [--only NAME ...]     one version: run the scenarios, write the record
  python tools/split_formats_trace.py --compare A.json B.json [C.json ...]               same traces?  same hashes?

--package: the directory that holds the `snuffy_amd` to import (default: this checkout); one process serves one version.  The loaded
library object is wrapped: per call of a C entry the record keeps its name, every integer and float argument, and null / non-null per
pointer.  Per scenario it keeps a SHA-256 of every output (results, gradients, parameters after the step).  Same seeds in every
scenario; nothing here times anything (--time measures host + device time of the same scenarios: ms per call, median of --rounds).

Scenarios: the fused fp32 training step at (16384, 768, h 6, Lambda 200) on the hl chain and on the forced cat chain, module in eval
and in train mode, and with encoder dropout (hl chain); the same step at (700, 256, h 4, Lambda 50); the fp32 eval forward at an
hl-eligible bag and at one that is not; the fp32 ViT-S/16 extractor at a chip-filling batch and at batch 2; one DINO and one MAE
frozen-trunk step (ViT-S/16 at 64 tiles, ViT-B/16 at batch 64: the rows of tools/vit_trunk_train_time.py).
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class TracedLib:
    """The library object with every call written to `log` (a list the owner swaps per scenario)."""

    def __init__(self, lib):
        self._lib, self._fns, self.log = lib, {}, None

    def __getattr__(self, name):
        fn = self._fns.get(name)
        if fn is None:
            real = getattr(self._lib, name)

            def fn(*args, _real=real, _name=name):
                if self.log is not None:
                    self.log.append([_name] + [describe(a) for a in args])
                return _real(*args)

            self._fns[name] = fn
        return fn


def describe(a):
    if a is None:
        return "null"
    if isinstance(a, bool):
        return int(a)
    if isinstance(a, int):
        return a
    if isinstance(a, float):
        return repr(a)
    if isinstance(a, ctypes.c_void_p):
        return "ptr" if a.value else "null"
    return type(a).__name__                                     # byref(...) and the like: an out-parameter


def digest(t):
    import torch
    if t is None:
        return None
    t = t.detach().contiguous().cpu()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()[:16]


def scenarios(dev):
    """name -> function returning [(label, tensor)]; every function seeds what it draws."""
    import torch
    from snuffy_amd import autograd as SA, ssl_pretrain as S, vit
    from snuffy_amd.snuffy import build_milnet
    from snuffy_amd.train import BagParallelStepper
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import vit_trunk_train_time as VT

    def milnet(d, h, lam, dropout=0.0):
        torch.manual_seed(0)
        net = build_milnet(d, h, "relu", lam, 0.0, 1, encoder_dropout=dropout)
        for p in net.parameters():
            if p.dim() > 1:
                torch.nn.init.xavier_normal_(p)
        return net.to(dev).configure(precision="fp32", return_attention=False)

    def bag(n, d, seed=1):
        return torch.randn(1, n, d, generator=torch.Generator().manual_seed(seed)).to(dev)

    def train(n, d, h, lam, hl, mode, dropout=0.0):
        def run():
            shipped = SA.X3_TRAIN_HL
            SA.X3_TRAIN_HL = hl
            try:
                net = milnet(d, h, lam, dropout)
                stepper = BagParallelStepper(net, device=dev, precision="fp32")
                net.train(mode == "train")
                x, y = bag(n, d), torch.tensor([1.0], device=dev)
                torch.manual_seed(4)                            # the dropout draws
                out = []
                for i in range(2):
                    ins, logits, _ = net(x)
                    fused = SA.mil_loss(ins, logits, y, stepper.w, stepper.criterion)       # BagParallelStepper.step, gradients kept
                    loss = fused[0] if fused is not None else (stepper.w * stepper.criterion(logits.view(1, -1), y.view(1, -1)) + (1 - stepper.w)
                                                               * stepper.criterion(torch.max(ins, 1)[0].view(1, -1), y.view(1, -1)))
                    loss.backward()
                    out += [("loss%d" % i, loss)] + [("grad%d.%s" % (i, k), p.grad) for k, p in net.named_parameters()]
                    stepper.optimizer.step()
                    stepper.optimizer.zero_grad()
                return out + [("param.%s" % k, p) for k, p in net.named_parameters()]
            finally:
                SA.X3_TRAIN_HL = shipped
        return run

    def evalfwd(n, d, h, lam):
        def run():
            net = milnet(d, h, lam).eval()
            with torch.no_grad():
                ins, logits, _ = net(bag(n, d))
                ins2, logits2, _ = net(bag(n, d, seed=2))       # the second forward finds the weight images cached
            return [("ins", ins), ("logits", logits), ("ins2", ins2), ("logits2", logits2)]
        return run

    def extractor(batch):
        def run():
            torch.manual_seed(0)
            model = vit.vit_small(patch_size=16, adapter_ffn_scalar="10", adapter_ffn_num=32, adapter_d_model=384).to(dev).eval().configure("fp32")
            x = torch.rand(batch, 3, 224, 224, generator=torch.Generator().manual_seed(6)).to(dev)
            with torch.no_grad():
                return [("features", model(x)), ("again", model(x))]
        return run

    def trunk(make):
        def run():
            fn = make()
            torch.manual_seed(5)
            return [("loss", torch.as_tensor(fn())), ("loss2", torch.as_tensor(fn()))]
        return run

    big, small = (16384, 768, 6, 200), (700, 256, 4, 50)
    return {
        "train_big_hl_eval": train(*big, True, "eval"), "train_big_hl_train": train(*big, True, "train"),
        "train_big_hl_train_encdrop": train(*big, True, "train", 0.1),
        "train_big_cat_eval": train(*big, False, "eval"), "train_big_cat_train": train(*big, False, "train"),
        "train_small_eval": train(*small, True, "eval"), "train_small_train": train(*small, True, "train"),
        "eval_hl_bag": evalfwd(16384, 768, 6, 200), "eval_cat_bag": evalfwd(700, 256, 4, 50),
        "vit_s16_batch512": extractor(512), "vit_s16_batch2": extractor(2),
        "dino_trunk_step": trunk(lambda: VT.dino_step(S, vit, torch, dev, 16)), "mae_trunk_step": trunk(lambda: VT.mae_step(S, torch, dev)),
    }


def run_version(args):
    sys.path.insert(0, os.path.abspath(args.package))
    import torch
    import snuffy_amd
    from snuffy_amd import _ffi
    assert os.path.dirname(os.path.dirname(os.path.abspath(snuffy_amd.__file__))) == os.path.abspath(args.package), snuffy_amd.__file__
    lib = TracedLib(_ffi.load())
    _ffi._lib = lib                                             # what every later _ffi.load() returns
    dev = torch.device("cuda:0")
    table = scenarios(dev)
    record = {"package": os.path.abspath(args.package), "scenarios": {}}
    for name in args.only or table:
        torch.cuda.empty_cache()
        if args.time:
            fn = table[name]
            fn()
            ts = []
            for _ in range(args.rounds):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append(1e3 * (time.perf_counter() - t0))
            record["scenarios"][name] = {"ms": sorted(ts)}
            print("%-28s ms %s" % (name, " ".join("%.2f" % t for t in sorted(ts))), flush=True)
            continue
        lib.log = []
        outs = table[name]()
        torch.cuda.synchronize()
        calls, lib.log = lib.log, None
        record["scenarios"][name] = {"calls": calls, "hashes": [[k, digest(t)] for k, t in outs]}
        print("%-28s %5d calls  %4d outputs" % (name, len(calls), len(outs)), flush=True)
        del outs
    json.dump(record, open(args.out, "w"))
    return 0


def compare(paths):
    """The first file is the baseline's first run; files whose `package` equals its package are further baseline runs (they say which
    hashes the baseline itself reproduces), the others are held against it."""
    recs = [json.load(open(p)) for p in paths]
    base = recs[0]
    twins = [r for r in recs[1:] if r["package"] == base["package"]]
    others = [(p, r) for p, r in zip(paths[1:], recs[1:]) if r["package"] != base["package"]]
    bad = 0
    for name, b in base["scenarios"].items():
        stable = {k for k, v in b["hashes"] if all(dict(t["scenarios"][name]["hashes"]).get(k) == v for t in twins)}
        unstable = [k for k, _ in b["hashes"] if k not in stable]
        for path, r in others:
            o = r["scenarios"].get(name)
            if o is None:
                print("%-28s %s: scenario missing" % (name, path))
                bad += 1
                continue
            same_trace = o["calls"] == b["calls"]
            if not same_trace:
                at = next((i for i, (x, y) in enumerate(zip(b["calls"], o["calls"])) if x != y), min(len(b["calls"]), len(o["calls"])))
                print("%-28s %s: TRACE DIFFERS at call %d: %s | %s" % (name, path, at, b["calls"][at:at + 1], o["calls"][at:at + 1]))
            oh = dict(o["hashes"])
            diff = [k for k, v in b["hashes"] if k in stable and oh.get(k) != v]
            print("%-28s %s: %d calls %s, %d of %d outputs hash as the baseline's%s%s"
                  % (name, os.path.basename(path), len(o["calls"]), "identical" if same_trace else "DIFFERENT", len(stable) - len(diff), len(stable),
                     (" -- DIFFERENT: " + ", ".join(diff[:6])) if diff else "",
                     (" -- the baseline does not reproduce itself at: " + ", ".join(unstable[:6])) if unstable else ""))
            bad += (not same_trace) + bool(diff)
    print("RESULT: %s" % ("identical traces and hashes wherever the baseline reproduces itself" if not bad else "%d differences" % bad))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package", default=ROOT)
    ap.add_argument("--out")
    ap.add_argument("--only", nargs="*")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--compare", nargs="+")
    args = ap.parse_args()
    if args.compare:
        return compare(args.compare)
    return run_version(args)


if __name__ == "__main__":
    sys.exit(main())
