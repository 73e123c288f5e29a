#!/usr/bin/env python
"""The collect phase of the turn-based Hanabi runner on one MI355X -- 100 buffer steps (one move per player each), policy
on the device, no update -- with the tables on the host (libhanabi_batch.so + one staged upload per move: the default)
and in device memory (--use_device_env: K16), timed in the same process, alternating.  Two shapes:

    sh        train_hanabi_forward.sh's: Hanabi-Full, 2 players, 1,000 tables, hidden 512 x 2 layers
    config5   BASELINE.json configs[4]: Hanabi-Full, 5 players, 8,192 tables, hidden 512 x 2 layers

    python tools/hanabi_rollout.py [--shapes sh,config5] [--reps 10] [--warmup 1] [--kernel_stats DIR] [--out file.json]
    rocprofv3 --kernel-trace --stats -f csv -o hanabi -d DIR/config5 -- python tools/hanabi_rollout.py --kernels_only --shapes config5

Per way: median, 10th / 90th percentile and range of the phase's wall time (host clock around work that ends in a device
synchronise) over ``--reps`` alternating repetitions after ``--warmup`` untimed ones.  ``spread_s`` is the larger of the
two 10th-to-90th-percentile widths; the device tables count as faster only if their median is lower by more than that.
Both ways start from the same seeds and weights and every repetition continues its way's games; the policy's sampling
draws from one generator shared by the two, so the games differ in detail and each way's move count is reported.

``--kernels_only`` runs a few device moves per shape and nothing else: the run to put under the profiler, on its own.
``--kernel_stats DIR`` reads the ``*kernel_stats.csv`` the profiler left under DIR/<shape> (one profiler run per shape)
and adds, for the encode kernel (the memory-bound one of a move's two launches), the bytes a launch writes -- computed
from the shapes: tables x (observation + centralised row + legal moves) x 4 -- over its average time, as a share of the
HBM peak (8.0 TB/s).  Prints one JSON line.
"""
import argparse
import csv
import glob
import json
import os
import pathlib
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "on-policy_amd"))

SHAPES = {"sh": dict(players=2, tables=1000), "config5": dict(players=5, tables=8192)}
HBM_PEAK_BYTES_PER_S = 8.0e12
STEPS = 100


def summary(s):
    q = statistics.quantiles(s, n=10) if len(s) > 1 else [s[0]] * 9
    return {"median_s": round(statistics.median(s), 4), "p10_s": round(q[0], 4), "p90_s": round(q[8], 4),
            "min_s": round(min(s), 4), "max_s": round(max(s), 4), "all_s": [round(x, 4) for x in s]}


def build_runner(shape, on_device, steps):
    import numpy as np
    import torch
    from onpolicy.config import get_config
    from onpolicy.runner.shared.hanabi_runner_forward import HanabiRunner
    from onpolicy.scripts.train import _launch, train_hanabi_forward
    argv = ["--env_name", "Hanabi", "--hanabi_name", "Hanabi-Full", "--num_agents", str(shape["players"]),
            "--algorithm_name", "mappo", "--experiment_name", "rollout", "--seed", "1", "--n_training_threads", "1",
            "--n_rollout_threads", str(shape["tables"]), "--episode_length", str(steps), "--num_env_steps", "1",
            "--hidden_size", "512", "--layer_N", "2", "--use_ReLU", "--use_wandb"] + (["--use_device_env"] if on_device else [])
    all_args = _launch.apply_algorithm_flags(train_hanabi_forward.parse_args(argv, get_config()), ("rmappo", "mappo", "ippo"))
    device = torch.device("cuda", 0)
    torch.manual_seed(1)
    np.random.seed(1)
    envs = train_hanabi_forward.make_env(all_args, all_args.n_rollout_threads, lambda rank: 1 + rank * 1000,
                                         device=device if on_device else None)
    run_dir = tempfile.mkdtemp()
    runner = HanabiRunner({"all_args": all_args, "envs": envs, "eval_envs": None, "num_agents": shape["players"],
                           "device": device, "run_dir": pathlib.Path(run_dir)})
    runner.begin_rollout()
    return runner


def collect_phase(runner, steps):
    for step in range(steps):
        runner.collect(step)
        runner.insert_and_restart()


def row_bytes(env):
    b = env.batch
    return 4 * (b.obs_len + b.players + b.share_len + b.players + b.num_moves)


def kernel_stats(directory):
    """{kernel name: (calls, average ns)} from the profiler's kernel statistics file(s) under ``directory``."""
    found = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row.get("Name") or row.get("KernelName") or ""
            calls = float(row.get("Calls") or 0)
            total = float(row.get("TotalDurationNs") or 0)
            if calls and total:
                found[name] = (int(calls), total / calls)
    return found


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="sh,config5")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=STEPS)
    ap.add_argument("--kernels_only", action="store_true")
    ap.add_argument("--kernel_stats", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    os.environ.setdefault("MAPPO_RESULTS_DIR", tempfile.mkdtemp())
    import torch
    assert torch.cuda.is_available(), "a timing needs the GPU"
    out = {"what": "wall time of the collect phase (%d buffer steps, no update), host tables and device tables "
                   "alternating, %d repetitions after %d warm-up each" % (opt.steps, opt.reps, opt.warmup),
           "commit": opt.commit, "hbm_peak_TB_per_s": HBM_PEAK_BYTES_PER_S / 1e12, "shapes": {}}

    def write():
        if opt.out:
            os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
            with open(opt.out, "w") as f:
                f.write(json.dumps(out) + "\n")

    for name in opt.shapes.split(","):
        shape = SHAPES[name]
        if opt.kernels_only:
            runner = build_runner(shape, True, 2)
            collect_phase(runner, 2)
            torch.cuda.synchronize()
            continue
        runners = {"host": build_runner(shape, False, opt.steps), "device": build_runner(shape, True, opt.steps)}

        def timed(way):
            torch.cuda.synchronize()
            a = time.perf_counter()
            collect_phase(runners[way], opt.steps)
            torch.cuda.synchronize()
            return time.perf_counter() - a

        for _ in range(opt.warmup):
            timed("host"), timed("device")
        times, moves = {"host": [], "device": []}, {}
        for way in times:
            moves[way] = -runners[way].true_total_num_steps
        for _ in range(opt.reps):               # alternating: both ways see the same machine
            for way in ("host", "device"):
                times[way].append(timed(way))
                print("%s %s %.3f s" % (name, way, times[way][-1]), file=sys.stderr, flush=True)
        for way in times:
            moves[way] += runners[way].true_total_num_steps
        h, d = summary(times["host"]), summary(times["device"])
        spread = max(h["p90_s"] - h["p10_s"], d["p90_s"] - d["p10_s"])
        env = runners["device"].envs
        rec = {"config": "Hanabi-Full, %d players, %d tables, hidden 512 x 2, mappo, 1 x MI355X" % (shape["players"], shape["tables"]),
               "host": h, "device": d, "spread_s": round(spread, 4),
               "spread_is": "the larger of the two ways' 10th-to-90th-percentile widths",
               "device_faster_by_s": round(h["median_s"] - d["median_s"], 4),
               "device_faster_than_spread": bool(h["median_s"] - d["median_s"] > spread),
               "host_moves_per_repetition": moves["host"] / float(opt.reps),
               "device_moves_per_repetition": moves["device"] / float(opt.reps),
               "host_moves_per_s": round(moves["host"] / sum(times["host"]), 1),
               "device_moves_per_s": round(moves["device"] / sum(times["device"]), 1),
               "host_ms_per_buffer_step": round(1e3 * h["median_s"] / opt.steps, 3),
               "device_ms_per_buffer_step": round(1e3 * d["median_s"] / opt.steps, 3),
               "row_bytes_per_table": row_bytes(env), "encode_bytes_per_launch": row_bytes(env) * shape["tables"]}
        if opt.kernel_stats:
            stats = kernel_stats(os.path.join(opt.kernel_stats, name))
            rec["kernel_stats_note"] = "average kernel times of a profiler run of its own at this shape (a few moves)"
            for key, tag in (("hanabi_encode_kernel", "encode"), ("hanabi_apply_kernel", "apply"), ("hanabi_deal_kernel", "deal")):
                hit = [(n, v) for n, v in stats.items() if key in n]
                if hit:
                    rec[tag + "_kernel_calls"], rec[tag + "_kernel_avg_us"] = hit[0][1][0], round(hit[0][1][1] / 1e3, 2)
            if "encode_kernel_avg_us" in rec:
                rate = rec["encode_bytes_per_launch"] / (rec["encode_kernel_avg_us"] * 1e-6)
                rec["encode_TB_per_s"] = round(rate / 1e12, 3)
                rec["encode_share_of_hbm_peak"] = round(rate / HBM_PEAK_BYTES_PER_S, 3)
        out["shapes"][name] = rec
        write()
        for r in runners.values():
            r.envs.close()
        del runners
        torch.cuda.empty_cache()
    print(json.dumps(out))
