#!/usr/bin/env python
"""One Hanabi evaluation (``HanabiRunner._eval_games``: every eval table played to the end with the deterministic policy),
three ways in one process, alternating: on the host stepper (the default), on device-resident eval tables eagerly
(--use_device_eval, MAPPO_EVAL_GRAPH=0) and with every move replayed from a captured graph (--use_device_eval).  Shapes of
tools/hanabi_rollout.py: ``sh`` (the reference eval script's: Hanabi-Full, 2 players, 1,000 tables, recurrent policy) and
``config5`` (5 players, 8,192 tables, feed-forward), hidden 512 x 2, freshly initialised weights (the same in every way).

    python tools/hanabi_device_eval.py [--shapes sh,config5] [--reps 10] [--warmup 1] [--kernel_trace DIR] [--out file.json]
    rocprofv3 --kernel-trace -f csv -o trace -d DIR/sh/captured -- python tools/hanabi_device_eval.py --kernels_only captured --shapes sh --out DIR/sh/captured/moves.json

Per way: median, 10th / 90th percentile and range of one evaluation's wall time over ``--reps`` alternating repetitions
after ``--warmup`` untimed ones (the first device evaluation builds the graphs); ``spread_s`` is the widest of the ways'
10th-to-90th-percentile widths, and one way counts as faster than another only if its median is lower by more than that.
Every repetition deals new games (the tables' generators continue), the same ones in every way; with freshly initialised
weights they are short, so the moves per evaluation are reported beside the times.  The captured way is timed again with
``MAPPO_HANABI_EVAL_POLL`` = 1, 2, 4, 8 (alternating): rounds of A moves between two reads of the counter block.

``--kernels_only WAY`` runs one evaluation of one way between two ``hanabi_draws_kernel`` launches (markers in the trace) and
nothing else: the run to put under the profiler, on its own (``--out``: the moves it played).  ``--kernel_trace DIR`` reads the
kernel traces and ``moves.json`` such runs left under DIR/<shape>/<way> and adds the launches per move (every launch of the evaluation -- the reset included -- over rounds x
players) and the average time of K18's two launches beside the bytes they move when every table moves.
Prints one JSON line.
"""
import argparse
import json
import os
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import hanabi_rollout as base           # noqa: E402  (shapes, summary(); puts the package on sys.path)
import hanabi_device_turns as turns     # noqa: E402  (between_markers())

WAYS = ("host", "eager", "captured")
POLLS = (1, 2, 4, 8)
ALGORITHM = {"sh": "rmappo", "config5": "mappo"}


def build_runner(name, shape, way):
    import pathlib
    import numpy as np
    import torch
    from onpolicy.config import get_config
    from onpolicy.runner.shared.hanabi_runner_forward import HanabiRunner
    from onpolicy.scripts.train import _launch, train_hanabi_forward
    argv = ["--env_name", "Hanabi", "--hanabi_name", "Hanabi-Full", "--num_agents", str(shape["players"]),
            "--algorithm_name", ALGORITHM[name], "--experiment_name", "eval", "--seed", "1", "--n_training_threads", "1",
            "--n_rollout_threads", "1", "--episode_length", "8", "--num_env_steps", "1", "--hidden_size", "512",
            "--layer_N", "2", "--use_ReLU", "--use_wandb", "--use_eval", "--n_eval_rollout_threads", str(shape["tables"])] + \
        ([] if way == "host" else ["--use_device_eval"])
    all_args = _launch.apply_algorithm_flags(train_hanabi_forward.parse_args(argv, get_config()), ("rmappo", "mappo", "ippo"))
    device = torch.device("cuda", 0)
    torch.manual_seed(1)
    np.random.seed(1)
    envs = train_hanabi_forward.make_env(all_args, 1, lambda rank: 1 + rank * 1000)
    eval_envs = train_hanabi_forward.make_env(all_args, shape["tables"], lambda rank: 50000 + rank * 10000,
                                              device=None if way == "host" else device)
    runner = HanabiRunner({"all_args": all_args, "envs": envs, "eval_envs": eval_envs, "num_agents": shape["players"],
                           "device": device, "run_dir": pathlib.Path(tempfile.mkdtemp())})
    runner.way = way
    return runner


def evaluate(runner, poll=None):
    """One ``_eval_games()`` -> (seconds, mean score)."""
    import numpy as np
    import torch
    os.environ["MAPPO_EVAL_GRAPH"] = "1" if runner.way == "captured" else "0"       # read when the first evaluation builds
    if poll is None:
        os.environ.pop("MAPPO_HANABI_EVAL_POLL", None)
    else:
        os.environ["MAPPO_HANABI_EVAL_POLL"] = str(poll)
    torch.cuda.synchronize()
    a = time.perf_counter()
    scores = runner._eval_games()
    torch.cuda.synchronize()
    b = time.perf_counter()
    if runner.way != "host":
        assert (runner.device_eval.graphs is not None) == (runner.way == "captured")
    return b - a, float(np.mean(scores))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="sh,config5")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--kernels_only", default=None, choices=WAYS[1:])
    ap.add_argument("--kernel_trace", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    os.environ.setdefault("MAPPO_RESULTS_DIR", tempfile.mkdtemp())
    import torch
    from onpolicy.runner.shared import hanabi_eval
    assert torch.cuda.is_available(), "a timing needs the GPU"
    out = {"what": "wall time of one Hanabi evaluation (_eval_games: every eval table played to the end, deterministic policy, "
                   "freshly initialised weights): host stepper, device eval eager, device eval captured, alternating, %d "
                   "repetitions after %d warm-up each; then the captured way with MAPPO_HANABI_EVAL_POLL in %s"
                   % (opt.reps, opt.warmup, list(POLLS)),
           "commit": opt.commit, "default_poll": hanabi_eval.DEFAULT_POLL, "shapes": {}}

    def write():
        if opt.out:
            os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
            with open(opt.out, "w") as f:
                f.write(json.dumps(out) + "\n")

    for name in opt.shapes.split(","):
        shape = base.SHAPES[name]
        if opt.kernels_only:
            runner = build_runner(name, shape, opt.kernels_only)
            evaluate(runner)                                # past first-call effects; builds the graphs
            runner.eval_envs.batch.draws()                  # marker
            evaluate(runner)
            runner.eval_envs.batch.draws()                  # marker
            torch.cuda.synchronize()
            out = {"shape": name, "way": opt.kernels_only, "rounds": runner.device_eval.rounds,
                   "moves_played": runner.device_eval.rounds * shape["players"]}
            write()                                         # (--out DIR/<shape>/<way>/moves.json: read by --kernel_trace)
            break                                           # one shape per profiled run
        runners = {way: build_runner(name, shape, way) for way in WAYS}
        for _ in range(opt.warmup):
            for way in WAYS:
                evaluate(runners[way])
        times, means, moves, rounds = {way: [] for way in WAYS}, {way: [] for way in WAYS}, [], []
        for _ in range(opt.reps):               # alternating: all ways see the same machine and play the same games
            for way in WAYS:
                t, mean = evaluate(runners[way])
                times[way].append(t)
                means[way].append(mean)
                print("%s %s %.3f s, mean score %.3f" % (name, way, t, mean), file=sys.stderr, flush=True)
            route = runners["captured"].device_eval
            moves.append(int(route.counters["moves"].sum()))
            rounds.append(route.rounds)
        s = {way: base.summary(times[way]) for way in WAYS}
        spread = max(s[way]["p90_s"] - s[way]["p10_s"] for way in WAYS)
        by_poll = {p: [] for p in POLLS}
        for _ in range(opt.reps):
            for p in POLLS:
                by_poll[p].append(evaluate(runners["captured"], poll=p)[0])
        sp = {p: base.summary(by_poll[p]) for p in POLLS}
        poll_spread = max(sp[p]["p90_s"] - sp[p]["p10_s"] for p in POLLS)
        best = min(POLLS, key=lambda p: sp[p]["median_s"])
        gain = s["eager"]["median_s"] - s["captured"]["median_s"]
        route, tables, A = runners["captured"].device_eval, shape["tables"], shape["players"]
        rnn_w = route.ops.rnn_states.shape[2] * route.ops.rnn_states.shape[3] if route.ops.recurrent else 0
        rec = {"config": "Hanabi-Full, %d players, %d eval tables, hidden 512 x 2, %s, 1 x MI355X"
                         % (A, tables, ALGORITHM[name]),
               "host_eval": s["host"], "device_eval_eager": s["eager"], "device_eval_captured": s["captured"],
               "spread_s": round(spread, 4), "spread_is": "the widest of the three ways' 10th-to-90th-percentile widths",
               "games_per_s": {way: round(tables / s[way]["median_s"], 1) for way in WAYS},
               "captured_faster_than_eager_by_s": round(gain, 4),
               "captured_beats_eager_by_more_than_spread": bool(gain > spread),
               "captured_faster_than_host_by_s": round(s["host"]["median_s"] - s["captured"]["median_s"], 4),
               "eager_faster_than_host_by_s": round(s["host"]["median_s"] - s["eager"]["median_s"], 4),
               "mean_scores_equal_in_every_way": bool(means["host"] == means["eager"] == means["captured"]),
               "mean_score_per_repetition": means,
               "moves_per_evaluation": moves, "rounds_per_evaluation_captured": rounds,
               "max_moves_by_the_rules": route.max_moves,
               "captured_by_poll": {str(p): sp[p] for p in POLLS}, "poll_spread_s": round(poll_spread, 4),
               "best_poll": best,
               "best_poll_beats_the_others_by_more_than_spread": bool(all(
                   sp[p]["median_s"] - sp[best]["median_s"] > poll_spread for p in POLLS if p != best)),
               "eval_begin_bytes_per_launch_all_moving": tables * (2 * 4 * rnn_w + 4 + 8 + 4),
               "eval_end_bytes_per_launch_none_finishing": tables * (4 + 4 + 4 + 2 * 8)}
        if opt.kernel_trace:
            rec["kernel_trace_note"] = "kernel-trace runs of their own at this shape, one evaluation between two markers"
            for way in WAYS[1:]:
                span = turns.between_markers(os.path.join(opt.kernel_trace, name, way))
                info = os.path.join(opt.kernel_trace, name, way, "moves.json")
                if span is None or not os.path.exists(info):
                    continue
                played = json.load(open(info))["moves_played"]
                rec["launches_per_move_" + way] = round(len(span) / float(played), 1)
                for kernel in ("hanabi_eval_begin_kernel", "hanabi_eval_end_kernel"):
                    d = [dur for n, dur in span if kernel in n]
                    if d:
                        rec[kernel + "_calls_" + way], rec[kernel + "_avg_us_" + way] = len(d), round(sum(d) / len(d) / 1e3, 2)
        out["shapes"][name] = rec
        write()
        for r in runners.values():
            r.envs.close()
            r.eval_envs.close()
        del runners
        torch.cuda.empty_cache()
    print(json.dumps(out))
