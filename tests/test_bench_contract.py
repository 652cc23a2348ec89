"""The bench line's contract: the newest committed end-of-round line (profiles/r*_bench_cfgB.json, printed by
`python bench.py --full` on an MI355X) carries every field the driver and the judge read, with consistent arithmetic; the launcher
logic of `--gpus N` (self-spawn, refusal of a mismatched world) and the --dump-outputs writer work without a GPU; on an MI355X a
plain run is the headline leg alone and dumps the same outputs run after run."""
import glob
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_refuses_a_world_that_is_not_gpus():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], env=env, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode != 0 and "--gpus 2 but WORLD_SIZE=1" in (out.stderr + out.stdout)


def test_bench_gpus_n_spawns_n_ranks():
    """No WORLD_SIZE in the environment: `--gpus 2` re-executes itself under torch.distributed.run with two ranks (which then stop
    at the GPU check here: the launcher ran, both ranks started)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"], env=env,
                         capture_output=True, text=True, timeout=600)
    text = out.stderr + out.stdout
    assert out.returncode != 0
    assert text.count("bench.py needs an MI355X") >= 2 or "local_rank: 1" in text or "rank: 1" in text, text[-2000:]


def test_committed_bench_line_has_the_contract_fields():
    path = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_bench_cfgB.json")))[-1]
    with open(path) as f:
        line = json.loads(f.read().strip().splitlines()[-1])
    if line["dtype"] == "f32":          # round 3 on: the reference's arithmetic is the headline, bf16 rides beside it
        assert line["value_bf16"] > 0 and line["value_f32_library_gemm"] > 0 and line["value_with_attention_output"] > 0
        assert line["roofline"]["kernel"].startswith(("sparse_attn_x3_kernel", "sparse_attn_x3p_kernel"))
        assert line["roofline_bf16"]["kernel"].startswith("sparse_attn_mfma_kernel")
        assert line["vit_bf16"]["value"] > 0 and line["vit_f32"]["value"] > 0 and line["vit_bf16"]["roofline"]["bound"] == "mfma"
        line = dict(line, dtype="bf16", value_f32=line["value"], roofline=line["roofline_bf16"], roofline_f32=line["roofline"])
    with open(os.path.join(ROOT, "BASELINE.json")) as f:
        base = json.load(f)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in line, key
    assert line["unit"] == "slides/s" and line["higher_is_better"] is True and line["scaling"] == "weak"
    assert line["vs_baseline"] is None and line["data"] == "synthetic" and line["n_gpus"] == 1
    assert "slides/sec" in str(base.get("metric", "")) and line["metric"] == "slides/sec"
    assert "workload" in line["config"] and "model" not in line["config"]
    assert "N=32768" in line["config"]["workload"] and "D=768" in line["config"]["workload"]
    # value is the whole-job rate of EXACTLY `steps` timed steps
    assert abs(line["value"] - line["n_gpus"] * 1e3 / line["ms_per_step"]) / line["value"] < 2e-3
    # both arithmetics in one driver-run line
    assert line["dtype"] == "bf16" and line["value_f32"] > 0 and line["value_f32_library_gemm"] > 0
    assert line["value_with_attention_output"] > 0
    for name in ("roofline", "roofline_f32"):
        r = line[name]
        for key in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "us_per_launch", "algorithmic_bytes"):
            assert key in r, (name, key)
        assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
        assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
        assert abs(r["achieved"] - r["algorithmic_bytes"] / (r["us_per_launch"] * 1e-6) / 1e9) / r["achieved"] < 2e-3
        assert r["traffic"] is None or r["traffic"] >= r["algorithmic_bytes"]
    assert line["roofline"]["kernel"].startswith("sparse_attn_mfma_kernel")
    assert line["roofline_f32"]["kernel"].startswith(("sparse_attn_x3_kernel", "sparse_attn_x3p_kernel"))     # the kernel the fp32 model dispatches
    cpu = line["cpu_baseline"]
    for key in ("value", "unit", "cores", "kind", "sample"):
        assert key in cpu, key
    assert cpu["kind"] == "port" and cpu["unit"] == "slides/s"
    sweep = cpu["thread_sweep"]
    assert cpu["value"] == max(sweep.values()) and str(cpu["cores"]) == max(sweep, key=sweep.get)


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("snf_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_writes_float_arrays_within_the_budget(tmp_path, monkeypatch):
    """--dump-outputs: one DIR/<name>.npy per output in float32 (float64 kept); above the budget every array is cut to the same
    fixed, seeded sample of its elements, identical from run to run."""
    import numpy as np
    import torch
    bench = _bench_module()
    outs = {"classes": torch.arange(12, dtype=torch.float32).view(1, 12, 1), "prediction_bag": torch.tensor([[0.25]], dtype=torch.bfloat16),
            "exact": torch.tensor([1.0 / 3.0], dtype=torch.float64)}
    assert bench.dump_outputs(outs, str(tmp_path / "a")) == ["classes", "exact", "prediction_bag"]
    c = np.load(tmp_path / "a" / "classes.npy")
    assert c.dtype == np.float32 and c.shape == (1, 12, 1) and np.array_equal(c.reshape(-1), np.arange(12))
    assert np.load(tmp_path / "a" / "prediction_bag.npy").dtype == np.float32
    assert np.load(tmp_path / "a" / "exact.npy").dtype == np.float64
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4000)
    big = {"w": torch.randn(3000, generator=torch.Generator().manual_seed(0)), "b": torch.ones(1000)}
    bench.dump_outputs(big, str(tmp_path / "b"))
    bench.dump_outputs(big, str(tmp_path / "c"))
    w1, w2 = np.load(tmp_path / "b" / "w.npy"), np.load(tmp_path / "c" / "w.npy")
    assert w1.nbytes + np.load(tmp_path / "b" / "b.npy").nbytes <= 4000 and w1.size == 750
    assert np.array_equal(w1, w2) and np.isin(w1, big["w"].numpy()).all()


def _run_plain_bench(args, out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "cfgA", "--preroll-s", "0.1",
           "--dump-outputs", str(out_dir)] + args
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])


def _cfga_bags():
    """bench.py's resident cfgA bags of rank 0 (seed 1234 + rank, eight of them), on the host."""
    import torch
    g = torch.Generator().manual_seed(1234)
    return [torch.randn(1, 8192, 384, generator=g) for _ in range(8)]


@pytest.mark.gpu
def test_plain_bench_run_is_the_headline_alone_and_dumps_the_same_outputs(tmp_path):
    """A plain run times exactly --steps steps of the headline leg and nothing else; --dump-outputs writes what its last timed
    step computed -- the eval forward of bag (warmup + steps - 1) % 8 -- and two runs with the same arguments write the same arrays."""
    import numpy as np
    import torch
    lines = [_run_plain_bench(["--steps", "5", "--warmup", "2"], tmp_path / d) for d in ("a", "b")]
    for line in lines:
        assert line["steps"] == 5 and line["warmup"] == 2 and line["ms_per_step"] > 0 and line["dtype"] == "f32"
        assert abs(line["value"] - 1e3 / line["ms_per_step"]) / line["value"] < 2e-3
        assert not any(k.startswith(("value_", "roofline", "vit_")) or k in ("cpu_baseline", "small_bags", "train_leg") for k in line)
    dumped = {}
    for name in ("classes", "prediction_bag"):
        a, b = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert a.dtype == np.float32 and np.array_equal(a, b), name
        dumped[name] = a
    # the same forward rebuilt here (bench.build_net: seeded weights), eager: graph replay is bit-identical to it
    bench = _bench_module()
    bags = _cfga_bags()
    net = bench.build_net(384, 6, 200, "fp32", torch.device("cuda", 0)).eval()
    with torch.no_grad():
        outs = {i: [t.cpu().numpy() for t in net(bags[i].cuda())[:2]] for i in (5, 6)}
    assert np.array_equal(dumped["classes"], outs[6][0]) and np.array_equal(dumped["prediction_bag"], outs[6][1])
    assert not np.array_equal(dumped["classes"], outs[5][0])          # another bag's forward would not pass


@pytest.mark.gpu
def test_plain_bench_train_dump_is_the_last_timed_step_and_repeats(tmp_path):
    """--mode train --dump-outputs: the timed region starts from the state the warm-up steps left, whatever the time-based
    pre-roll ran, so two runs dump the same loss and weights -- those of W + N training steps in a row from the seeded model."""
    import numpy as np
    import torch
    args = ["--mode", "train", "--steps", "3", "--warmup", "1", "--preroll-s", "0.3"]
    lines = [_run_plain_bench(args, tmp_path / d) for d in ("a", "b")]
    for line in lines:
        assert line["steps"] == 3 and "value_train" not in line
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b")) and "loss.npy" in files
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 * 10 ** 6
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float32 and np.array_equal(a, b), f
    # warm-up step 0, then the timed steps 1..3, straight through on a fresh seeded model (no pre-roll)
    from snuffy_amd.train import BagParallelStepper
    bench = _bench_module()
    dev = torch.device("cuda", 0)
    bags = _cfga_bags()
    net = bench.build_net(384, 6, 200, "fp32", dev)
    net.configure(return_attention=False, sampler="device")
    stepper = BagParallelStepper(net, world_size=1, dist=None, device=dev, precision="fp32")
    for i in range(4):
        loss = stepper.step(bags[i % 8].to(dev), torch.tensor([float(i % 2)], device=dev))
    torch.cuda.synchronize()
    np.testing.assert_allclose(np.load(tmp_path / "a" / "loss.npy"), loss.float().cpu().numpy(), rtol=1e-5, atol=0)
    params = dict(net.named_parameters())
    assert {f[len("param."):-len(".npy")] for f in files if f.startswith("param.")} == set(params)
    for k, p in params.items():      # one AdamW step more or less moves the weights by ~lr = 2e-4
        np.testing.assert_allclose(np.load(tmp_path / "a" / ("param." + k + ".npy")), p.detach().float().cpu().numpy(),
                                   rtol=0, atol=1e-6, err_msg=k)
