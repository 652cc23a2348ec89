"""BASELINE.json configs that round 1 left without a -m gpu test, and the fixture gaps of rows a-14 / a-12:
  configs[4]  CAMELYON16-scale lognormal slide set (bench.py --workload cam16) through Snuffy.train + valid, per-bag vs the oracle
  configs[3]  ViT-S/16 + adapter at batch 512 (sampled images vs the ViT oracle, whole batch vs sub-batches)
  a-14        Snuffy._run_model against the F3 fixtures (bag_pred, loss, sigmoid(c))
  a-12        bf16 GELU (erf in the reference) at config-A size against the erf oracle
  8e          BagParallelStepper (bench.py's train step) == one Snuffy.train step, bit for bit at world_size 1
"""
import json
import os

import numpy as np
import pytest
import torch

from oracle import snuffy_oracle as orc
from oracle import vit_oracle as vorc
from tests.helpers import build_amd_milnet, golden_files, load_case, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _record(name, payload):
    """Measured error levels go to gpurun_out/ (scratch) so DESIGN.md can quote them."""
    try:
        os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
        with open(os.path.join(ROOT, "gpurun_out", "measured_%s.json" % name), "w") as f:
            json.dump(payload, f)
    except OSError:
        pass


def _snuffy_args(D, precision="fp32", **kw):
    from snuffy_amd.train import get_args_parser
    a = get_args_parser().parse_args([])
    a.feats_size, a.optimizer, a.num_epochs, a.precision = D, "adamw", 2, precision
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def cam16_lengths(n_bags=400, mean=30000, sigma=0.5, seed=0):
    """bench.py's cam16 generator."""
    rs = np.random.RandomState(seed)
    return np.clip(np.round(rs.lognormal(np.log(mean) - sigma * sigma / 2, sigma, n_bags)), 1000, 100000).astype(int)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_cam16_slide_set_through_trainer_vs_oracle(precision):
    """configs[4]: 12 slides of the 400-slide lognormal set (every N different, 9 k .. 75 k patches, D = 768) through
    Snuffy.valid (eval forward per bag) against the CPU oracle, then one Snuffy.train epoch over the same resident bags."""
    from snuffy_amd.train import Snuffy
    lens = cam16_lengths()[::34][:12]
    assert len(set(lens.tolist())) == 12
    torch.manual_seed(0)
    np.random.seed(0)
    tr = Snuffy(_snuffy_args(768, precision))
    sd = {k: v.detach().cpu().clone() for k, v in tr.milnet.state_dict().items()}
    g = torch.Generator().manual_seed(1234)
    bags = [torch.randn(int(n), 768, generator=g) for n in lens]
    labels = [np.array([float(i % 2)], dtype=np.float32) for i in range(len(bags))]
    staged = [b.unsqueeze(0).to(DEV) for b in bags]
    res = tr.valid((labels, staged, None, None))
    tol = 1e-3 if precision == "fp32" else 1e-2
    worst = 0.0
    with torch.no_grad():
        for i, b in enumerate(bags):
            classes_ref, logits_ref, _, sels = orc.milnet_forward(b, sd, 6, "relu", 200, 0.0, 1)
            pred_ref = 0.5 * torch.sigmoid(classes_ref.max()) + 0.5 * torch.sigmoid(logits_ref.squeeze())
            _, logits, _ = tr.milnet(staged[i])
            worst = max(worst, float((logits.cpu().view(-1) - logits_ref.view(-1)).abs().max()))
            assert abs(float(res["predictions"][i, 0]) - float(pred_ref)) < tol, (i, int(lens[i]))
            top, _ = tr.milnet.b_classifier.encoder.layers[0].last_selection
            if precision == "fp32":      # scores differ from the oracle's only in the last bits: same selected SET
                assert set(top.cpu().tolist()) == set(sels[0].tolist()), int(lens[i])
    assert worst < tol, worst
    _record("cam16_%s" % precision, {"max_abs_logit_err": worst, "lens": lens.tolist()})
    out = tr.train((labels, staged, None, None), 1)
    assert sorted(out["visited"]) == list(range(12)) and np.isfinite(out["epoch_train_loss"])
    assert out["predictions"].shape == (12, 1)


def test_vit_small_adapter_batch_512():
    """configs[3]: DINO ViT-S/16 + adapter (ffn_num 32, scalar 10) at batch 512, 224 x 224: 8 sampled images against the ViT
    oracle, and the whole batch against itself run in sub-batches of 4 (batch-size independence of every kernel)."""
    from snuffy_amd import vit
    torch.manual_seed(0)
    model = vit.vit_small(patch_size=16, adapter_ffn_scalar="10", adapter_ffn_num=32, adapter_d_model=384)
    with torch.no_grad():                      # the LoRA init leaves the adapter at zero: give it (and every bias) weight
        for n_, p in model.named_parameters():
            if "adaptmlp.up_proj" in n_ or n_.endswith(".bias"):
                p.normal_(0.0, 0.02)
    emb = vit.IClassifier(model, 384, 2).to(DEV).eval()
    x = torch.rand(512, 3, 224, 224, generator=torch.Generator().manual_seed(3)).to(DEV)
    sample = [0, 1, 63, 130, 255, 256, 400, 511]
    sd = {k: v.cpu() for k, v in model.state_dict().items()}
    ref = vorc.vit_forward(x[sample].cpu(), sd, 16, 12, 6, 10.0, "dino_adapter")
    measured = {}
    for precision, tol in (("fp32", 1e-3), ("bf16", 1e-2)):
        model.configure(precision)
        with torch.no_grad():
            feats, c = emb(x)
            sub = torch.cat([emb(x[i:i + 4])[0] for i in range(0, 512, 4)])
        assert feats.shape == (512, 384) and c.shape == (512, 2)
        err = float((feats[sample].cpu().float() - ref).abs().max())
        rerr = rel_err(feats[sample].cpu().float(), ref)
        bdiff = float((feats.float() - sub.float()).abs().max())
        measured[precision] = {"max_abs_err": err, "rel_err": rerr, "batch_vs_subbatch": bdiff,
                               "ref_absmax": float(ref.abs().max())}
        # fp32: a batch of 512 takes the one-pass x3 GEMM kernel, sub-batches of 4 the concatenated form (both fp32-class, different
        # summation order) -- equal to ~1e-5 of the feature scale, not bit for bit
        assert bdiff <= (1e-4 if precision == "fp32" else tol), (precision, bdiff)
        # north-star tolerance classes: 1e-3 fp32, 1e-2 bf16 -- on features normalised by their own scale (the final
        # LayerNorm puts them at O(1); max |feat| is recorded next to the error)
        assert rerr < tol, (precision, err, rerr)
    _record("vit_b512", measured)


@pytest.mark.parametrize("path", golden_files("f3_"), ids=lambda p: p.split("/")[-1][:-4])
def test_run_model_hook_against_f3(path):
    """a-14: the trainer hook Snuffy._run_model (reference train.py:828-846, 913-916) returns the reference's
    (bag_pred, loss, sigmoid(c).view(-1, 1))."""
    from snuffy_amd.train import Snuffy
    z, sd = load_case(path)
    N, D, h, lam, depth, seed = [int(v) for v in z["cfg"]]
    tr = Snuffy(_snuffy_args(D, num_heads=h, big_lambda=lam, depth=depth, activation=str(z["act"]),
                             random_patch_share=float(z["r"])))
    tr.milnet.load_state_dict(sd, strict=True)
    tr.milnet.eval()                                   # the fixture was captured with the dropouts off
    x = torch.from_numpy(z["x"]).to(DEV)
    y = torch.from_numpy(z["y"]).to(DEV)
    np.random.seed(seed)
    bag_pred, loss, ins_sigmoid = tr._run_model(x, y)
    assert float(tr.single_weight_parameter) == 0.5
    np.testing.assert_allclose(float(bag_pred), float(z["bag_pred"]), rtol=0, atol=1e-5)
    np.testing.assert_allclose(loss.item(), float(z["loss"]), rtol=0, atol=1e-5)
    assert tuple(ins_sigmoid.shape) == tuple(z["ins_sigmoid"].shape) == (N, 1)
    np.testing.assert_allclose(ins_sigmoid.detach().cpu().numpy(), z["ins_sigmoid"], rtol=0, atol=1e-5)


def test_bf16_gelu_at_config_a_vs_erf_oracle():
    """a-12: the reference's FFN activation is nn.GELU() = the erf form (snuffy.py:218).  The bf16 path at config-A size
    (N = 8192, D = 384, hidden 1536) against the erf oracle: logits and A inside the bf16 class."""
    torch.manual_seed(0)
    N, D, h, lam = 8192, 384, 6, 200
    net = build_amd_milnet(D, h, "gelu", lam, 0.0, 1)
    for _, p in net.named_parameters():
        if p.dim() > 1:
            torch.nn.init.xavier_normal_(p)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    x = torch.randn(N, D, generator=torch.Generator().manual_seed(8))
    _, logits_ref, p_ref, _ = orc.milnet_forward(x, sd, h, "gelu", lam, 0.0, 1)
    net = net.to(DEV).eval()
    errs = {}
    for precision, tol in (("fp32", 1e-3), ("bf16", 1e-2)):
        net.configure(precision=precision, return_attention=True)
        with torch.no_grad():
            _, logits, A = net(x.to(DEV).unsqueeze(0))
        errs[precision] = float((logits.cpu()[0] - logits_ref).abs().max())
        assert errs[precision] < tol and float((A.cpu()[0] - p_ref).abs().max()) < tol
    _record("gelu_cfgA", errs)


def test_bag_parallel_stepper_equals_trainer_step_world1():
    """at world_size 1 the bag-parallel step bench.py times IS the reference's step-per-bag -- the post-step weights
    of BagParallelStepper.step and of one Snuffy.train iteration are bit-identical."""
    from snuffy_amd.train import BagParallelStepper, Snuffy
    D = 128
    args = _snuffy_args(D, num_heads=2, big_lambda=32, weight_decay=5e-3)
    torch.manual_seed(1)
    tr = Snuffy(args)
    for m in tr.milnet.modules():                  # attention dropout off: both steps must draw nothing random
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    import copy
    twin = copy.deepcopy(tr.milnet)
    x = torch.randn(1, 700, D, generator=torch.Generator().manual_seed(2)).to(DEV)
    label = np.array([1.0], dtype=np.float32)
    np.random.seed(3)
    tr.train(([label], [x], None, None), 1)
    st = BagParallelStepper(twin, world_size=1, dist=None, device=DEV, lr=args.lr, betas=tuple(args.betas),
                            weight_decay=args.weight_decay, precision="fp32")
    # the trainer applies dropout_patches (a row permutation at p = 0) before the forward: replay the same draws
    from snuffy_amd.utils import dropout_patches_device
    np.random.seed(3)
    from sklearn.utils import shuffle
    shuffle(np.arange(1))                           # the epoch order consumed one draw first
    xp = dropout_patches_device(x, 0.0)
    st.optimizer = type(tr.optimizer)(params=[{"params": twin.parameters()}], lr=args.lr, betas=tuple(args.betas),
                                      weight_decay=args.weight_decay, fused=True)   # as the trainer builds it on the GPU
    st.step(xp, torch.tensor([1.0], device=DEV))
    for (k, a), (_, b) in zip(tr.milnet.named_parameters(), twin.named_parameters()):
        assert torch.equal(a, b), k


@pytest.mark.parametrize("p", [0.0, 0.2, 0.5])
@pytest.mark.parametrize("batched", [False, True])
def test_dropout_patches_device_replays_reference(p, batched):
    """utils.dropout_patches_device -- what Trainer.train applies to HBM-resident bags -- against the reference's own output (F5,
    reference utils.py:244-250): the same rows bit for bit AND the same position of the global numpy RNG stream afterwards."""
    from snuffy_amd.utils import dropout_patches_device
    z = np.load(golden_files("f5_")[0])
    feats = torch.from_numpy(z["feats"]).to(DEV)
    if batched:
        feats = feats.unsqueeze(0)
    np.random.seed(11)
    out = dropout_patches_device(feats, p)
    assert out.is_cuda and out.dim() == feats.dim()
    got = out[0] if batched else out
    assert np.array_equal(got.cpu().numpy(), z[f"out_p{p}"])
    assert np.random.rand() == float(z[f"next_rand_p{p}"])          # the next draw of the stream is the reference's


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_bench_rccl_path_on_one_rank(mode):
    """bench.py as the driver launches it for N > 1 (torch.distributed.run, one rank per GPU), here with one rank and the RCCL
    process group forced on: init, barriers, the max-over-ranks all-reduce, the per-rank all-gather and -- in train mode -- the
    flat-gradient all-reduce all run on the real backend (an N > 1 run is the driver's)."""
    import subprocess
    import sys
    env = dict(os.environ, SNF_BENCH_FORCE_DIST="1", MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", "29541" if mode == "eval" else "29542", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "cfgA",
           "--steps", "6", "--warmup", "2", "--full", "--headline-only", "--no-cpu-baseline", "--no-roofline", "--mode", mode,
           "--precision", "bf16"]
    out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["config"]["rccl_ranks"] == 1 and line["n_gpus"] == 1 and line["value"] > 0
    assert len(line["config"]["per_rank_slides_per_s"]) == 1


def test_bag_parallel_two_ranks_on_rccl(tmp_path):
    """SURVEY 8e on the device (VERDICT r5 #4 / #5a): two ranks on the "nccl" (= RCCL) backend, the REAL model.  One
    BagParallelStepper step at world 2 (rank r on bag r, ONE flat-gradient all-reduce) == one process that accumulates both bags'
    gradients, halves them and steps; the replicas stay bit-identical; sharded Snuffy.valid == the single-process pass.  Needs two
    GPUs: skipped on a one-GPU box (the driver's multi-GPU node runs it)."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs >= 2 GPUs (torch.cuda.device_count() = %d)" % torch.cuda.device_count())
    import subprocess
    import sys
    out_path = str(tmp_path / "world2.pt")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29547", os.path.join(ROOT, "tests", "nccl_world2_worker.py"), out_path]
    run = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    if run.returncode != 0 and not os.path.exists(out_path) and any(t in run.stderr for t in ("ncclSystemError", "ncclUnhandled", "hipIpc", "RendezvousError")):
        pytest.skip("two visible GPUs, but RCCL could not be brought up between them on this box: " + run.stderr[-400:])
    assert run.returncode == 0, run.stderr[-3000:]
    z = torch.load(out_path, weights_only=False)
    r0, r1 = z["ranks"]
    for k in r0["after"]:
        assert torch.equal(r0["after"][k], r1["after"][k]), k                       # replicas never drift
    assert np.array_equal(r0["preds"], r1["preds"]) and r0["loss"] == r1["loss"]
    # single-process reference: same start weights, both bags accumulated at half weight, one AdamW step
    from snuffy_amd.train import BagParallelStepper, Snuffy
    args = _snuffy_args(128, num_heads=2, big_lambda=32)
    torch.manual_seed(1)
    tr = Snuffy(args)
    tr.milnet.load_state_dict(z["start"])
    for m in tr.milnet.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    st = BagParallelStepper(tr.milnet, world_size=1, dist=None, device=DEV, lr=args.lr, betas=tuple(args.betas),
                            weight_decay=args.weight_decay, precision="fp32")
    for bag, label in zip(z["bags"], z["labels"]):
        ins, logits, _ = tr.milnet(bag.to(DEV))
        max_pred, _ = torch.max(ins, 1)
        y = label.to(DEV)
        loss = st.w * st.criterion(logits.view(1, -1), y.view(1, -1)) + (1 - st.w) * st.criterion(max_pred.view(1, -1), y.view(1, -1))
        (loss / 2).backward()
    st.optimizer.step()
    for k, v in tr.milnet.state_dict().items():
        ref = v.detach().cpu()
        scale = max(1e-6, float(ref.abs().max()))
        assert float((r0["after"][k] - ref).abs().max()) <= 2e-6 * scale + 1e-9, k   # (g0 + g1) / 2 in either association
    tr.milnet.load_state_dict(r0["after"])
    res = tr.valid((z["vlabels"], z["vfeats"], None, None))
    assert np.allclose(res["predictions"], r0["preds"], atol=1e-6) and abs(res["epoch_valid_loss"] - r0["loss"]) < 1e-6
