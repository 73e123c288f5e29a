"""-m gpu: bench.py's one-line JSON contract at a small size, and the data-parallel code path on RCCL
with a single rank (MAPPO_FORCE_DIST=1: flat gradient bucket, statistic all-reduces, barrier) --
the 8-GPU run itself is the driver's."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _run(extra_env=None, args=()):
    env = dict(os.environ)
    env.update(extra_env or {})
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--threads", "64", "--steps", "1",
                          "--warmup", "1", "--full", "--no-cpu-baseline", "--sampler-rng", "host"]
                         + ([] if "--gemm-tuning" in args else ["--no-gemm-tuning"])
                         + [a for a in args if a != "--gemm-tuning"],
                         capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    return json.loads(line)


def test_default_command_line_carries_the_other_baseline_configs():
    """`python bench.py --full` (north star, one GPU) appends `workloads`: the other BASELINE configs run by child processes of the same
    script after the timed region (VERDICT r5 "next" #1).  Here with two of the six (MAPPO_BENCH_WORKLOADS) to keep the test
    short: entries carry value / ms_per_step / arithmetic / the dominant launch against its roof / the GAE launch in situ."""
    env = dict(os.environ, MAPPO_BENCH_WORKLOADS="cfg2,smac_shard64", HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0", "--full",
                          "--no-cpu-baseline", "--no-f32-mfma"], capture_output=True, text=True, env=env, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1                      # ONE JSON line, whatever the children printed
    d = json.loads(lines[0])
    assert d["config"]["n_rollout_threads"] == 4096 and d["value"] > 0
    w = d["workloads"]
    assert set(w) == {"cfg2", "smac_shard64"}, w.keys()
    for name, e in w.items():
        assert "error" not in e and "skipped" not in e, (name, e)
        assert e["value"] > 0 and e["ms_per_step"] > 0 and e["dtype"] == "f32" and e["arithmetic"].startswith("f32 products")
        assert 0 < e["roofline"]["frac"] < 1 and e["roofline"]["bound"] in ("hbm", "mfma")
        assert 0 < e["roofline_gae"]["frac"] < 1
        assert e["update_graph_replays_per_step"] == 10.0      # both replay their ten updates per step from HIP graphs
    assert w["cfg2"]["n_rollout_threads"] == 1024 and w["smac_shard64"]["n_rollout_threads"] == 64
    assert d["update_graph_capture_failures"] == 0 and len(d["csrc_digest"]) == 16


def test_bench_contract_and_rccl_single_rank():
    plain = _run()
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                "scaling", "vs_baseline", "dtype", "data", "config", "roofline"):
        assert key in plain, key
    assert plain["unit"] == "env-steps/s" and plain["n_gpus"] == 1 and plain["data"] == "synthetic"
    assert plain["config"]["workload"] and "model" not in plain["config"]
    r = plain["roofline"]       # dominant kernel: the fused trunk's forward launch, against the nearer of its two roofs
    assert r["bound"] in ("mfma", "hbm") and r["unit"] == {"mfma": "TFLOP/s", "hbm": "GB/s"}[r["bound"]]
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and 0 < r["frac"] < 1
    assert r["frac"] == max(v["frac"] for v in r["roofs"].values()) and all(0 < v["frac"] < 1 for v in r["roofs"].values())
    assert r["launches"] == 20 and r["flop_per_launch"] > 0 and plain["roofline_mlp_backward"]["launches"] == 20
    g = plain["roofline_gae"]   # the kernel the north star names, HBM bound
    assert g["bound"] == "hbm" and g["unit"] == "GB/s" and abs(g["frac"] - g["achieved"] / g["peak"]) < 1e-3
    # (one timed step: one profiled GAE launch, timed by the event pair recorded around it)
    assert g["timing"].startswith("HIP event pair") and "event_pair_around_launch" not in g and g["launches"] == 1
    # from two timed steps on the launches alternate between that pair and the kernel's own begin / end timestamps (events
    # attached to the dispatch: mappo_gae_time_next_launch), which `frac` then quotes; the pair -- it also times two
    # command-processor packets -- is kept next to it and can only be the longer one
    g2 = _run(args=("--steps", "2", "--no-f32-mfma"))["roofline_gae"]
    pair = g2["event_pair_around_launch"]
    assert g2["timing"].startswith("kernel begin / end timestamps") and 0 < g2["launch_ms"] <= pair["launch_ms"] * 1.02
    assert g2["in_situ"]["frac"] == g2["frac"] and g2["in_situ"]["event_pair_around_launch"] == pair["frac"] and g2["launches"] == 1
    assert abs(g2["frac"] - g2["achieved"] / g2["peak"]) < 1e-3
    # the arithmetic of the timed region is named, and the float32-MFMA step of the SAME run sits next to `value` (VERDICT
    # r4's conditions for the six-term default); peak HBM per rank is reported
    assert plain["dtype"] == "f32" and plain["arithmetic"].startswith("f32 products from six bf16xbf16 terms of exact 3-way splits")
    f32 = plain["f32_mfma"]
    assert f32["value"] > 0 and f32["ms_per_step"] > 0 and f32["unit"] == plain["unit"] and "six_term" not in plain
    # six terms: the float32-equivalent matrix-core peak is the dense bf16 MFMA peak / 6
    assert r["roofs"]["mfma"]["peak"] == 416.7 and r["roofs"]["hbm"]["peak"] == 8000.0
    assert abs(r["frac_of_f32_mfma_peak"] - r["roofs"]["mfma"]["achieved"] / 157.3) < 1e-3
    assert len(plain["hbm_peak_bytes_per_rank"]) == 1 and plain["hbm_peak_bytes_per_rank"][0] > 1 << 20
    swapped = _run(args=("--matrix-arithmetic", "f32_mfma"))
    assert swapped["arithmetic"].startswith("f32 MFMA") and swapped["six_term"]["value"] > 0 and "f32_mfma" not in swapped
    assert swapped["roofline"]["roofs"]["mfma"]["peak"] == 157.3
    for k, v in plain["train_info"].items():        # same seeds and permutations: the two forms agree to float32 noise
        assert swapped["train_info"][k] == pytest.approx(v, rel=2e-3, abs=1e-5), k
    forced = _run({"MAPPO_FORCE_DIST": "1", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29577", "RANK": "0",
                   "WORLD_SIZE": "1", "LOCAL_RANK": "0"})
    # same seeds, same host permutations: the RCCL path must reproduce the plain update
    for k, v in plain["train_info"].items():
        assert forced["train_info"][k] == pytest.approx(v, rel=2e-3, abs=1e-5), k


def test_plain_line_and_dumped_outputs(tmp_path):
    """Without --full the line carries the headline figures and none of the per-launch ones; --dump-outputs writes what the
    last timed step computed (float32 / float64 .npy files, 64 MB at most), the same for two runs of one command line."""
    import numpy as np
    runs = []
    for i in range(2):
        d = tmp_path / str(i)
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--threads", "64", "--steps", "2", "--warmup", "1",
               "--sampler-rng", "host", "--no-gemm-tuning", "--dump-outputs", str(d)]
        out = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"),
                             timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        line = json.loads(lines[0])
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in line, key
        assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0 and line["dtype"] == "f32"
        assert not any(k.startswith("roofline") for k in line) and "cpu_baseline" not in line and "f32_mfma" not in line
        files = {f.name[:-4]: np.load(f) for f in d.glob("*.npy")}
        assert "returns" in files and any(k.startswith("actor.") for k in files) and any(k.startswith("critic.") for k in files)
        assert all(a.dtype in (np.float32, np.float64) for a in files.values())
        assert sum(f.stat().st_size for f in d.glob("*.npy")) <= 64 << 20
        for k, v in line["train_info"].items():
            assert float(files["train_info." + k]) == pytest.approx(v, rel=1e-5, abs=1e-6), k
        runs.append(files)
    assert sorted(runs[0]) == sorted(runs[1])
    for k in runs[0]:           # host permutations, same seeds: the same update
        np.testing.assert_allclose(runs[0][k], runs[1][k], rtol=1e-4, atol=1e-6, err_msg=k)


def test_two_ranks_on_one_gpu_strong_scaling_path():
    """The driver's multi-GPU launch line with 2 ranks, both mapped onto the one GPU of this box (gloo
    carries the collectives because RCCL refuses duplicate devices): sharding of the rollout threads,
    per-rank buffers, flat-bucket gradient all-reduce on device tensors, max-over-ranks timing and the
    single JSON line from rank 0."""
    env = dict(os.environ)
    env.update(MAPPO_DIST_BACKEND="gloo", MAPPO_SINGLE_DEVICE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29611", os.path.join(ROOT, "bench.py"),
           "--gpus", "2", "--steps", "1", "--warmup", "1", "--threads", "64", "--sampler-rng", "host", "--full"]
    out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines          # exactly one JSON line, from rank 0
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong"
    assert d["config"]["threads_per_gpu"] == 32 and d["config"]["n_rollout_threads"] == 64
    assert "cpu_baseline" not in d
    assert all(abs(v) < 1e6 for v in d["train_info"].values())


def test_plain_gpus_flag_runs_two_ranks():
    """`python bench.py --gpus 2` with NO launcher around it: bench.py starts the two ranks itself (both mapped onto
    this box's one GPU, gloo carrying the collectives) and rank 0's line reports n_gpus = 2; `--gpus 1` is one plain
    process as before."""
    env = dict(os.environ)
    env.update(MAPPO_DIST_BACKEND="gloo", MAPPO_SINGLE_DEVICE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--threads", "64", "--steps", "1",
                          "--warmup", "1", "--sampler-rng", "host", "--no-gemm-tuning", "--full"],
                         capture_output=True, text=True, env=env, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["threads_per_gpu"] == 32
    assert d["rccl_ranks"] == 0                       # gloo in this test mode; RCCL ranks are reported when nccl carries them
    assert d["grad_allreduce"]["per_step"] == 10 and d["grad_allreduce"]["bucket_bytes"] > 0
    one = _run(args=("--gpus", "1"))
    assert one["n_gpus"] == 1 and one["grad_allreduce"]["per_step"] == 0


def test_two_ranks_over_rccl_when_the_box_has_two_gpus():
    """The driver's multi-GPU line for real: `bench.py --gpus 2`, one rank per GPU, collectives on RCCL (backend "nccl")
    over xGMI.  Skipped on one-GPU boxes (every box of rounds 1-5); on the first multi-GPU box this runs inside the device
    suite: rank 0's line must report two RCCL ranks, ten gradient all-reduces per step, per-rank peak HBM -- and the sharded
    update must reproduce the single-GPU one (same seeds, host permutations are per rank, so compare the losses loosely)."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (RCCL refuses two ranks on one device)")
    env = dict(os.environ)
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MAPPO_DIST_BACKEND", "MAPPO_SINGLE_DEVICE"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--threads", "64", "--steps", "2",
                          "--warmup", "1", "--no-gemm-tuning", "--full"], capture_output=True, text=True, env=env, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["rccl_ranks"] == 2 and d["config"]["threads_per_gpu"] == 32
    assert d["grad_allreduce"]["per_step"] == 10 and d["grad_allreduce"]["bucket_bytes"] > 0
    assert len(d["hbm_peak_bytes_per_rank"]) == 2 and min(d["hbm_peak_bytes_per_rank"]) > 1 << 20
    one = _run(args=("--gpus", "1", "--sampler-rng", "device"))
    for k in ("value_loss", "policy_loss", "dist_entropy"):
        assert d["train_info"][k] == pytest.approx(one["train_info"][k], rel=5e-2, abs=1e-3), k


@pytest.mark.parametrize("args_over", [dict(), dict(use_policy_active_masks=False, use_valuenorm=False, use_huber_loss=False)],
                         ids=["default", "unmasked_nonorm_mse"])
def test_two_rank_device_update_equals_single_process(tmp_path, args_over):
    """Data parallelism on the device path (HBM buffer, fused loss with global denominators, flat gradient
    bucket): two ranks sharing GPU 0 over gloo, each with half of the rollout threads, must end with identical
    replicas that match the single-process update on the whole buffer (num_mini_batch = 1)."""
    import numpy as np
    import torch
    import torch.multiprocessing as mp
    import dp_worker
    from test_data_parallel_cpu import _free_port
    N, world, port = 6, 2, _free_port()
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=dp_worker.worker, args=(r, world, port, N, args_over, str(tmp_path), "cuda:0"))
             for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    ranks = [torch.load(os.path.join(str(tmp_path), "rank%d.pt" % r), weights_only=False) for r in range(world)]
    for k in ranks[0]["sd"]:
        assert torch.equal(ranks[0]["sd"][k], ranks[1]["sd"][k]), k
    info, sd, ws = dp_worker.run_update(N, 0, N, args_over, torch.device("cuda", 0))
    assert ws == 1
    for k in sd:
        np.testing.assert_allclose(ranks[0]["sd"][k].numpy(), sd[k].numpy(), rtol=2e-4, atol=5e-6, err_msg=k)
    for k in ("actor_grad_norm", "critic_grad_norm"):
        assert ranks[0]["info"][k] == pytest.approx(info[k], rel=1e-3, abs=1e-6)
    for k in ("value_loss", "policy_loss", "dist_entropy", "ratio"):     # mean over ranks of per-rank means
        assert ranks[0]["info"][k] == pytest.approx(ranks[1]["info"][k], rel=1e-6, abs=1e-9)


def test_two_rank_device_update_on_hidden64_reference_fixture(tmp_path):
    """Two ranks sharing GPU 0 (gloo), each with half of the rollout threads of the reference-generated north-star-flag
    case at hidden 64: HBM buffers, lazy-obs samplers, K9 forward / backward, fused loss with global denominators, one
    gradient all-reduce per update -- against the weights the REFERENCE's single process ended with."""
    from test_data_parallel_cpu import _two_ranks_on_reference_fixture
    _two_ranks_on_reference_fixture(tmp_path, "h64_ns", "cuda:0")


def test_two_rank_device_sampler_route_one_scalar_collective_per_train(tmp_path):
    """The same two ranks on the route bench.py times (sampler_rng=device: identity index list, whole-batch tuple handed
    out again in epoch 2): still the reference's weights, and the scalar prologue (loss denominators + ValueNorm moments)
    crossed the ranks ONCE for the whole train() -- the second update reused it (DataParallel.minibatch_scales)."""
    from test_data_parallel_cpu import _two_ranks_on_reference_fixture
    ranks = _two_ranks_on_reference_fixture(tmp_path, "h64_ns", "cuda:0", {"sampler_rng": "device"})
    for r in ranks:
        assert r["info"]["_whole_batch_reuses"] == 1
        assert r["info"]["_scalar_collectives"] == 1 and r["info"]["_scales_reused"] == 1, r["info"]


@pytest.mark.parametrize("cname", ["dev_relu2", "dev_gru"])
def test_two_rank_prologue_ahead_equals_prologue_in_line(tmp_path, monkeypatch, cname):
    """Several minibatches per epoch: the scalar all-reduce of minibatch i + 1 is issued before update i runs
    (R_MAPPO._with_prologue_ahead).  Same arithmetic on the same rows, so the replicas must end bit-identical to a run
    with the prologue in line (MAPPO_PROLOGUE_AHEAD=0), one scalar collective per update either way."""
    import torch
    from test_data_parallel_cpu import _run_two_ranks
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("MAPPO_PROLOGUE_AHEAD", mode)
        d = tmp_path / mode
        d.mkdir()
        spec, ranks = _run_two_ranks(d, cname, "cuda:0", {"sampler_rng": "device"}, fname="trainer_dev_cases")
        updates = spec["spec"]["args"]["ppo_epoch"] * spec["spec"]["args"]["num_mini_batch"]
        for k in ranks[0]["sd"]:
            assert torch.equal(ranks[0]["sd"][k], ranks[1]["sd"][k]), k
        assert all(r["info"]["_scalar_collectives"] == updates and r["info"]["_scales_reused"] == 0 for r in ranks)
        out[mode] = ranks[0]
    for k in out["1"]["sd"]:
        assert torch.equal(out["1"]["sd"][k], out["0"]["sd"][k]), k
    for k in ("value_loss", "policy_loss", "actor_grad_norm", "critic_grad_norm"):
        assert out["1"]["info"][k] == out["0"]["info"][k]


def test_gemm_tuning_preloads_shipped_winners(tmp_path):
    """onpolicy.utils.gemm_tuning: TunableOp comes up with the shipped winners for the bench shapes loaded (no
    tuning needed for them), and a bench run with it reports gemm_tuning = true."""
    import torch
    from onpolicy.utils import gemm_tuning
    assert os.path.exists(gemm_tuning.SHIPPED)
    os.environ["MAPPO_GEMM_TUNING_CACHE"] = str(tmp_path)
    os.environ["MAPPO_GEMM_TUNING"] = "1"        # the session default for tests is off (conftest.py)
    try:
        assert gemm_tuning.enable(tune_new=False)
        keys = {r[1] for r in gemm_tuning.results()}
        assert "tn_64_2621440_384_ld_384_384_64" in keys          # critic 384 -> 64 layer at the north-star span
        a = torch.randn(4096, 64, device="cuda")
        w = torch.randn(64, 64, device="cuda")
        torch.testing.assert_close(a @ w, (a.double() @ w.double()).float(), rtol=1e-4, atol=1e-4)
    finally:
        torch.cuda.tunable.enable(False)
        os.environ.pop("MAPPO_GEMM_TUNING_CACHE", None)
    out = _run({"MAPPO_GEMM_TUNING_CACHE": str(tmp_path), "MAPPO_GEMM_TUNING": "1"}, args=("--gemm-tuning",))
    assert out["config"]["gemm_tuning"] is True
