#!/usr/bin/env python
"""One ``runner.eval()`` of train_mpe.py on one MI355X with the training worlds on the device (--use_device_env, rmappo,
128 eval worlds, 25 steps, hidden 64), timed in the same process, alternating:

  host   simple_spread only: the parent commit's command line, ``--use_device_env --use_eval`` -- eval worlds on the host
         (numpy ``VecSimpleSpread``), observations up and actions down every step;
  eager  ``--use_device_eval`` with the eager tensor loop (what ``MAPPO_EVAL_GRAPH=0`` runs);
  graph  ``--use_device_eval`` with the step replayed from its captured graph (runner/shared/eval_graph.py,
         runner/separated/eval_graph.py).

simple_reference and simple_speaker_listener are timed the last two ways only: without the flag their eval worlds come
from an external env tree, so the parent commit cannot evaluate them from a clean checkout.

    python tools/device_eval.py [--reps 30] [--warmup 5] [--commit HASH] [--out file.json]

Per way: median, quartiles, 10th / 90th percentile and range of the call's wall time (host clock around a call that ends
in the one device-to-host copy of the totals; the call's prints go nowhere, its log writes are part of it) over ``--reps``
calls after ``--warmup`` untimed ones.  ``spread_ms`` is the larger of the eager and the graph way's
10th-to-90th-percentile widths; the captured step stays the default inside ``--use_device_eval`` only if its median is
below the eager loop's by more than that (the rule of tools/speaker_listener_rollout.py).  ``spread_with_host_ms`` also
counts the host way's width: what the gain over the host evaluation is read against.  Prints one JSON line.
"""
import argparse
import contextlib
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "on-policy_amd"))

SCENARIOS = (("simple_spread", "3", True), ("simple_reference", "2", False), ("simple_speaker_listener", "2", False))


def summary(ms):
    q = statistics.quantiles(ms, n=20)          # 5 % steps
    return {"median_ms": round(statistics.median(ms), 4), "p25_ms": round(q[4], 4), "p75_ms": round(q[14], 4),
            "p10_ms": round(q[1], 4), "p90_ms": round(q[17], 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "all_ms": [round(x, 4) for x in ms]}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=128)
    ap.add_argument("--episode_length", type=int, default=25)
    ap.add_argument("--hidden_size", type=int, default=64)
    ap.add_argument("--algorithm_name", default="rmappo")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--commit", default=None, help="commit the measurement was made on (recorded in the JSON line)")
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    os.environ.setdefault("MAPPO_RESULTS_DIR", tempfile.mkdtemp())
    os.environ["MAPPO_ROLLOUT_GRAPH"] = "1"
    os.environ["MAPPO_EVAL_GRAPH"] = "1"
    import torch
    from onpolicy.scripts.train import train_mpe
    assert torch.cuda.is_available(), "a timing needs the GPU"
    T, N = opt.episode_length, opt.threads

    def runner_of(scenario, agents, flags):
        argv = ["--env_name", "MPE", "--algorithm_name", opt.algorithm_name, "--experiment_name", "check",
                "--scenario_name", scenario, "--num_agents", agents, "--num_landmarks", "3", "--seed", "1",
                "--n_training_threads", "1", "--n_rollout_threads", str(N), "--num_mini_batch", "1",
                "--episode_length", str(T), "--num_env_steps", str(T * N), "--ppo_epoch", "15", "--gain", "0.01",
                "--lr", "7e-4", "--critic_lr", "7e-4", "--hidden_size", str(opt.hidden_size), "--use_wandb",
                "--log_interval", "1000", "--save_interval", "1000", "--use_device_env", "--use_eval",
                "--n_eval_rollout_threads", str(N), "--eval_interval", "1000"]
        if scenario == "simple_speaker_listener":
            argv.append("--share_policy")       # store_false: one policy per agent
        # one whole iteration: builds everything, one train(), one evaluation (which captures the eval step)
        return train_mpe.main(argv + list(flags))

    def timed(call):
        torch.cuda.synchronize()
        with open(os.devnull, "w") as null, contextlib.redirect_stdout(null):
            a = time.perf_counter()
            call()
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - a)

    out = {"config": "train_mpe.py MPE, %s, n_rollout_threads=%d, n_eval_rollout_threads=%d, episode_length=%d, "
                     "hidden_size=%d, --use_device_env --use_eval, 1 x MI355X" % (opt.algorithm_name, N, N, T, opt.hidden_size),
           "commit": opt.commit,
           "what": "wall time of one runner.eval() (%d steps of %d worlds), %d alternating repetitions after %d warm-up "
                   "calls each" % (T, N, opt.reps, opt.warmup),
           "ways": {"host": "the parent commit's command line (no --use_device_eval): eval worlds on the host",
                    "eager": "--use_device_eval, MAPPO_EVAL_GRAPH=0: the eager tensor loop",
                    "graph": "--use_device_eval: the captured step, one graph launch per step"},
           "spread_is": "the larger of the eager and the graph way's 10th-to-90th-percentile widths "
                        "(spread_with_host_ms: of all three ways')", "scenarios": {}}
    for scenario, agents, with_host in SCENARIOS:
        dev = runner_of(scenario, agents, ["--use_device_eval"])
        graph = dev.eval_graph
        assert graph is not None and graph.graph is not None, "the eval step was not captured"
        steps = [0]

        def device_eval(g):
            dev.eval_graph = g
            steps[0] += 1
            dev.eval(10 ** 6 + steps[0])

        ways = {"eager": lambda: device_eval(None), "graph": lambda: device_eval(graph)}
        if with_host:
            host = runner_of(scenario, agents, [])
            assert type(host.eval_envs).__name__ == "VecSimpleSpread"
            ways = dict(host=lambda: host.eval(10 ** 6), **ways)
        for _ in range(opt.warmup):
            for call in ways.values():
                timed(call)
        times = {k: [] for k in ways}
        replays = graph.replays
        for _ in range(opt.reps):               # alternating: every way sees the same machine
            for k, call in ways.items():
                times[k].append(timed(call))
        assert graph.replays == replays + opt.reps * T
        dev.eval_graph = graph
        s = {k: summary(v) for k, v in times.items()}
        spread = max(s[k]["p90_ms"] - s[k]["p10_ms"] for k in ("eager", "graph"))
        rec = dict(s, spread_ms=round(spread, 4),
                   graph_faster_than_eager_by_ms=round(s["eager"]["median_ms"] - s["graph"]["median_ms"], 4),
                   graph_is_default=bool(s["eager"]["median_ms"] - s["graph"]["median_ms"] > spread),
                   eager_ms_per_env_step=round(s["eager"]["median_ms"] / T, 4),
                   graph_ms_per_env_step=round(s["graph"]["median_ms"] / T, 4))
        if with_host:
            rec["spread_with_host_ms"] = round(max(v["p90_ms"] - v["p10_ms"] for v in s.values()), 4)
            rec["graph_faster_than_host_by_ms"] = round(s["host"]["median_ms"] - s["graph"]["median_ms"], 4)
            rec["host_over_graph"] = round(s["host"]["median_ms"] / s["graph"]["median_ms"], 2)
            rec["host_ms_per_env_step"] = round(s["host"]["median_ms"] / T, 4)
        else:
            rec["host"] = None
            rec["host_note"] = ("not timed: without --use_device_eval the eval worlds of this scenario come from an "
                                "external env tree (MAPPO_ENVS_PATH), so the parent commit cannot evaluate it from a "
                                "clean checkout")
        out["scenarios"][scenario] = rec
    out["graph_is_default"] = all(v["graph_is_default"] for v in out["scenarios"].values())
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as f:
            f.write(json.dumps(out) + "\n")
    print(json.dumps(out))
