#!/usr/bin/env python
"""The collect phase of the turn-based Hanabi runner with the tables on the device, three ways in one process,
alternating: the default device route (--use_device_env: the host decides who moves, one flags copy per move), the
host-free route eagerly (--use_device_turns, MAPPO_TURN_GRAPH=0) and the host-free route with every move replayed from a
captured graph (--use_device_turns).  Protocol and shapes of tools/hanabi_rollout.py: collect phase only, 100 buffer
steps, ``sh`` (Hanabi-Full, 2 players, 1,000 tables) and ``config5`` (5 players, 8,192 tables), hidden 512 x 2.

    python tools/hanabi_device_turns.py [--shapes sh,config5] [--reps 10] [--warmup 1] [--kernel_trace DIR] [--out file.json]
                                        [--recurrent]
    rocprofv3 --kernel-trace -f csv -o trace -d DIR/config5/default -- python tools/hanabi_device_turns.py --kernels_only default --shapes config5
    rocprofv3 --kernel-trace -f csv -o trace -d DIR/config5/captured -- python tools/hanabi_device_turns.py --kernels_only captured --shapes config5

Per way: median, 10th / 90th percentile and range of the phase's wall time over ``--reps`` alternating repetitions after
``--warmup`` untimed ones; ``spread_s`` is the widest of the ways' 10th-to-90th-percentile widths, and the captured route
counts as faster than the default device route only if its median is lower by more than that.  All ways start from the
same seeds and weights; the host-free route samples other trajectories than the default route (its noise tensor is
[N, moves], not [movers, moves]), so each way's move count is reported.

``--kernels_only WAY`` runs a few buffer steps of one way between two ``hanabi_draws_kernel`` launches (markers in the
trace) and nothing else: the run to put under the profiler, on its own.  ``--kernel_trace DIR`` reads the kernel traces
such runs left under DIR/<shape>/<way> and adds the launches per player move of both routes (every launch of a buffer
step -- chooseinsert, reset and merge included -- over steps x players) and, for ``turn_begin`` (the memory-bound launch
of K17), its bytes -- 2 x tables x row bytes -- over its average time as a share of the HBM peak (8.0 TB/s).
``--recurrent``: the same three ways with the recurrent policy of the reference's eval script (rmappo, hidden 512 x 2,
recurrent_N 1); the host-free ways then also take ``--use_device_turns_rnn`` and K17's two launches keep the actor's and the
critic's RNN state (profiles/hanabi_device_turns_rnn.json).  ``turn_begin`` then moves 2 x rnn_w more floats per table.
Prints one JSON line.
"""
import argparse
import csv
import glob
import json
import os
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import hanabi_rollout as base       # noqa: E402  (shapes, summary(), row_bytes(); puts the package on sys.path)

WAYS = ("default", "eager", "captured")
KERNEL_STEPS = 4
MARKER = "hanabi_draws_kernel"


def build_runner(shape, way, steps, recurrent=False):
    import pathlib
    import numpy as np
    import torch
    from onpolicy.config import get_config
    from onpolicy.runner.shared.hanabi_runner_forward import HanabiRunner
    from onpolicy.scripts.train import _launch, train_hanabi_forward
    argv = ["--env_name", "Hanabi", "--hanabi_name", "Hanabi-Full", "--num_agents", str(shape["players"]),
            "--algorithm_name", "rmappo" if recurrent else "mappo", "--experiment_name", "rollout", "--seed", "1",
            "--n_training_threads", "1", "--n_rollout_threads", str(shape["tables"]), "--episode_length", str(steps), "--num_env_steps", "1",
            "--hidden_size", "512", "--layer_N", "2", "--use_ReLU", "--use_wandb", "--use_device_env"] + \
        ([] if way == "default" else ["--use_device_turns"] + (["--use_device_turns_rnn"] if recurrent else []))
    all_args = _launch.apply_algorithm_flags(train_hanabi_forward.parse_args(argv, get_config()), ("rmappo", "mappo", "ippo"))
    device = torch.device("cuda", 0)
    torch.manual_seed(1)
    np.random.seed(1)
    envs = train_hanabi_forward.make_env(all_args, all_args.n_rollout_threads, lambda rank: 1 + rank * 1000, device=device)
    runner = HanabiRunner({"all_args": all_args, "envs": envs, "eval_envs": None, "num_agents": shape["players"],
                           "device": device, "run_dir": pathlib.Path(tempfile.mkdtemp())})
    os.environ["MAPPO_TURN_GRAPH"] = "1" if way == "captured" else "0"      # read when begin_rollout builds the graphs
    runner.begin_rollout()
    assert (runner.route.name == "device_turns") == (way != "default") and (runner.turn_graphs is not None) == (way == "captured")
    assert bool(runner.policy.actor._recurrent) == recurrent and (way == "default" or runner.route.ops.recurrent == recurrent)
    return runner


def collect_phase(runner, steps):
    for step in range(steps):
        runner.collect(step)
        runner.insert_and_restart()


def moves_so_far(runner):
    runner.route.score_summary()
    return runner.true_total_num_steps


def between_markers(directory):
    """[kernel name, duration ns] of every dispatch between the last two marker launches of the trace under ``directory``."""
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row.get("Kernel_Name") or row.get("KernelName") or row.get("Name") or ""
            start = int(row.get("Start_Timestamp") or row.get("BeginNs") or 0)
            end = int(row.get("End_Timestamp") or row.get("EndNs") or 0)
            rows.append((start, name, end - start))
    rows.sort()
    marks = [i for i, r in enumerate(rows) if MARKER in r[1]]
    if len(marks) < 2:
        return None
    return [(name, dur) for _, name, dur in rows[marks[-2] + 1:marks[-1]]]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="sh,config5")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=base.STEPS)
    ap.add_argument("--kernels_only", default=None, choices=WAYS)
    ap.add_argument("--recurrent", action="store_true", help="the recurrent policy (rmappo); host-free ways with --use_device_turns_rnn")
    ap.add_argument("--kernel_trace", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    os.environ.setdefault("MAPPO_RESULTS_DIR", tempfile.mkdtemp())
    import torch
    assert torch.cuda.is_available(), "a timing needs the GPU"
    out = {"what": "wall time of the collect phase (%d buffer steps, no update) with the tables on the device: default "
                   "device route, device turns eager, device turns captured, alternating, %d repetitions after %d warm-up "
                   "each%s" % (opt.steps, opt.reps, opt.warmup, "; recurrent policy (--use_device_turns_rnn)" if opt.recurrent else ""),
           "commit": opt.commit, "hbm_peak_TB_per_s": base.HBM_PEAK_BYTES_PER_S / 1e12, "shapes": {}}

    def write():
        if opt.out:
            os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
            with open(opt.out, "w") as f:
                f.write(json.dumps(out) + "\n")

    for name in opt.shapes.split(","):
        shape = base.SHAPES[name]
        if opt.kernels_only:
            runner = build_runner(shape, opt.kernels_only, KERNEL_STEPS, opt.recurrent)
            collect_phase(runner, KERNEL_STEPS)             # past first-call effects
            runner.envs.batch.draws()                       # marker
            collect_phase(runner, KERNEL_STEPS)
            runner.envs.batch.draws()                       # marker
            torch.cuda.synchronize()
            continue
        runners = {way: build_runner(shape, way, opt.steps, opt.recurrent) for way in WAYS}

        def timed(way):
            torch.cuda.synchronize()
            a = time.perf_counter()
            collect_phase(runners[way], opt.steps)
            torch.cuda.synchronize()
            return time.perf_counter() - a

        for _ in range(opt.warmup):
            for way in WAYS:
                timed(way)
        times = {way: [] for way in WAYS}
        moves = {way: -moves_so_far(runners[way]) for way in WAYS}
        for _ in range(opt.reps):               # alternating: all ways see the same machine
            for way in WAYS:
                times[way].append(timed(way))
                print("%s %s %.3f s" % (name, way, times[way][-1]), file=sys.stderr, flush=True)
        for way in WAYS:
            moves[way] += moves_so_far(runners[way])
        s = {way: base.summary(times[way]) for way in WAYS}
        spread = max(s[way]["p90_s"] - s[way]["p10_s"] for way in WAYS)
        env = runners["default"].envs
        # what turn_begin moves per table: the three rows and, for a recurrent policy, the two new states
        state_bytes = 2 * 4 * runners["default"].turn.rnn_states[0, 0].numel() if opt.recurrent else 0
        policy = "rmappo (recurrent, recurrent_N 1)" if opt.recurrent else "mappo"
        gain = s["default"]["median_s"] - s["captured"]["median_s"]
        rec = {"config": "Hanabi-Full, %d players, %d tables, hidden 512 x 2, %s, 1 x MI355X" % (shape["players"], shape["tables"], policy),
               "default_device_route": s["default"], "device_turns_eager": s["eager"], "device_turns_captured": s["captured"],
               "spread_s": round(spread, 4), "spread_is": "the widest of the three ways' 10th-to-90th-percentile widths",
               "captured_faster_than_default_by_s": round(gain, 4),
               "captured_beats_default_by_more_than_spread": bool(gain > spread),
               "eager_faster_than_default_by_s": round(s["default"]["median_s"] - s["eager"]["median_s"], 4),
               "moves_per_repetition": {way: moves[way] / float(opt.reps) for way in WAYS},
               "ms_per_buffer_step": {way: round(1e3 * s[way]["median_s"] / opt.steps, 3) for way in WAYS},
               "ms_per_player_move": {way: round(1e3 * s[way]["median_s"] / opt.steps / shape["players"], 3) for way in WAYS},
               "row_bytes_per_table": base.row_bytes(env),
               "turn_begin_bytes_per_launch": 2 * (base.row_bytes(env) + state_bytes) * shape["tables"]}
        if opt.recurrent:
            rec["state_bytes_per_table"] = state_bytes
        if opt.kernel_trace:
            rec["kernel_trace_note"] = "kernel-trace runs of their own at this shape, %d buffer steps between two markers" % KERNEL_STEPS
            for way, key in (("default", "default_device_route"), ("captured", "device_turns_captured")):
                span = between_markers(os.path.join(opt.kernel_trace, name, way))
                if span is None:
                    continue
                rec["launches_per_player_move_" + key] = round(len(span) / float(KERNEL_STEPS * shape["players"]), 1)
                begin = [d for n, d in span if "hanabi_turn_begin_kernel" in n]
                if begin:
                    avg = sum(begin) / float(len(begin))
                    rate = rec["turn_begin_bytes_per_launch"] / (avg * 1e-9)
                    rec["turn_begin_kernel_calls"], rec["turn_begin_kernel_avg_us"] = len(begin), round(avg / 1e3, 2)
                    rec["turn_begin_TB_per_s"] = round(rate / 1e12, 3)
                    rec["turn_begin_share_of_hbm_peak"] = round(rate / base.HBM_PEAK_BYTES_PER_S, 3)
                end = [d for n, d in span if "hanabi_turn_end_kernel" in n]
                if end:
                    rec["turn_end_kernel_avg_us"] = round(sum(end) / float(len(end)) / 1e3, 2)
        out["shapes"][name] = rec
        write()
        for r in runners.values():
            r.envs.close()
        del runners
        torch.cuda.empty_cache()
    print(json.dumps(out))
