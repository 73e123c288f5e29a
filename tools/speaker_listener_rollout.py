#!/usr/bin/env python
"""One 25-step rollout of the reference's train_mpe_comm.sh (MPE simple_speaker_listener, 2 agents, 3 landmarks, rmappo,
128 rollout threads, hidden 64, one policy per agent) -- or, with ``--scenario simple_push --num_agents A --num_landmarks
L``, of keep-away at the same script family's shape, or, with ``--scenario simple_tag --num_adversaries V
--num_good_agents G --num_landmarks L``, of predator-prey, or, with ``--scenario simple_world_comm`` and the same three
flags, of predator-prey with forests, food and a speaking leader -- on one MI355X with the worlds on the device (--use_device_env),
timed two ways in the same process, alternating: the separated runner's eager device loop (collect -> envs.step ->
insert: what MAPPO_ROLLOUT_GRAPH=0 runs) and the captured step (runner/separated/rollout_graph.py: one graph launch + one
slab write per agent).  Both start every rollout from the buffers' row 0 and leave the same fields behind.

    python tools/speaker_listener_rollout.py [--reps 30] [--warmup 5] [--commit HASH] [--out file.json [--append]]
    python tools/speaker_listener_rollout.py --scenario simple_push --num_agents 3 --num_landmarks 2 ...
    python tools/speaker_listener_rollout.py --scenario simple_tag --num_adversaries 3 --num_good_agents 1 ...
    python tools/speaker_listener_rollout.py --scenario simple_world_comm --num_adversaries 4 --num_good_agents 2 \
        --num_landmarks 1 ...

Per way: median, quartiles, 10th / 90th percentile and range of the rollout's wall time (host clock around work that ends
in a device synchronise) over ``--reps`` rollouts after ``--warmup`` untimed ones.  ``spread_ms`` is the larger of the two
10th-to-90th-percentile widths; the captured step stays the default only if its median is below the eager loop's by more
than that.  ``eager_launches_per_step``: kernels of one eager step, ``eager_device_activities_per_step``: kernels, copies
and memsets together, both counted by the framework's profiler in a run of its own after the timing (null with the reason
where the profiler is not available).  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "on-policy_amd"))


def summary(ms):
    q = statistics.quantiles(ms, n=20)          # 5 % steps
    return {"median_ms": round(statistics.median(ms), 4), "p25_ms": round(q[4], 4), "p75_ms": round(q[14], 4),
            "p10_ms": round(q[1], 4), "p90_ms": round(q[17], 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "all_ms": [round(x, 4) for x in ms]}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenario", default="simple_speaker_listener", choices=("simple_speaker_listener", "simple_push", "simple_tag", "simple_world_comm"))
    ap.add_argument("--num_agents", type=int, default=2, help="simple_tag / simple_world_comm: --num_adversaries + --num_good_agents instead")
    ap.add_argument("--num_adversaries", type=int, default=3, help="simple_tag / simple_world_comm only")
    ap.add_argument("--num_good_agents", type=int, default=1, help="simple_tag / simple_world_comm only")
    ap.add_argument("--num_landmarks", type=int, default=None, help="default: 3 for simple_speaker_listener, 2 otherwise")
    ap.add_argument("--threads", type=int, default=128)
    ap.add_argument("--episode_length", type=int, default=25)
    ap.add_argument("--hidden_size", type=int, default=64)
    ap.add_argument("--algorithm_name", default="rmappo")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--commit", default=None, help="commit the measurement was made on (recorded in the JSON line)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="add the JSON line to --out (one line per shape) instead of replacing it")
    opt = ap.parse_args()
    landmarks = opt.num_landmarks if opt.num_landmarks is not None else (3 if opt.scenario == "simple_speaker_listener" else 2)
    tag = ["--num_adversaries", str(opt.num_adversaries), "--num_good_agents", str(opt.num_good_agents)]
    by_kind = opt.scenario in ("simple_tag", "simple_world_comm")        # adversaries followed by good agents
    if by_kind:
        opt.num_agents = opt.num_adversaries + opt.num_good_agents
    os.environ.setdefault("MAPPO_RESULTS_DIR", tempfile.mkdtemp())
    os.environ["MAPPO_ROLLOUT_GRAPH"] = "1"
    import torch
    from onpolicy.scripts.train import train_mpe
    assert torch.cuda.is_available(), "a timing needs the GPU"
    T, N = opt.episode_length, opt.threads
    argv = ["--env_name", "MPE", "--algorithm_name", opt.algorithm_name, "--experiment_name", "check",
            "--scenario_name", opt.scenario, "--num_agents", str(opt.num_agents), "--num_landmarks", str(landmarks),
            "--seed", "1",
            "--n_training_threads", "1", "--n_rollout_threads", str(N), "--num_mini_batch", "1",
            "--episode_length", str(T), "--num_env_steps", str(T * N), "--ppo_epoch", "15", "--gain", "0.01",
            "--lr", "7e-4", "--critic_lr", "7e-4", "--share_policy", "--hidden_size", str(opt.hidden_size), "--use_wandb",
            "--log_interval", "1000", "--save_interval", "1000", "--use_device_env"] + (tag if by_kind else [])
    runner = train_mpe.main(argv)           # one whole iteration: builds everything, captures the step, one train()
    graph = runner.rollout_graph
    assert graph is not None and graph.graph is not None, "the rollout step was not captured"
    for tr in runner.trainer:
        tr.prep_rollout()

    def eager_step(step):
        values, actions, logp, rnn_a, rnn_c, actions_env = runner.collect(step)
        obs, rewards, dones, infos = runner.envs.step(actions_env)
        runner.insert((obs, rewards, dones, infos, values, actions, logp, rnn_a, rnn_c))

    def eager():
        for step in range(T):
            eager_step(step)

    def graphed():
        graph.begin_episode()
        for step in range(T):
            graph.step()

    def timed(rollout):
        torch.cuda.synchronize()
        a = time.perf_counter()
        rollout()
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - a)
        for b in runner.buffer:             # row T becomes row 0 of the next rollout (outside the timed window)
            b.after_update()
        return ms

    for _ in range(opt.warmup):
        timed(eager), timed(graphed)
    times = {"eager": [], "graph": []}
    for _ in range(opt.reps):               # alternating: both ways see the same machine
        times["eager"].append(timed(eager))
        times["graph"].append(timed(graphed))
    e, g = summary(times["eager"]), summary(times["graph"])
    launches, activities, why = None, None, None
    spread = max(e["p90_ms"] - e["p10_ms"], g["p90_ms"] - g["p10_ms"])

    agents = ("%d agents" % opt.num_agents if not by_kind else
              "%d adversaries against %d good agents" % (opt.num_adversaries, opt.num_good_agents))
    out = {"config": "%s: MPE %s, %s, %d landmarks, %s, n_rollout_threads=%d, "
                     "episode_length=%d, hidden_size=%d, one policy per agent, 1 x MI355X, worlds on the device"
                     % ("train_mpe_comm.sh" if opt.scenario == "simple_speaker_listener" else "train_mpe.sh family",
                        opt.scenario, agents, landmarks, opt.algorithm_name, N, T, opt.hidden_size),
           "commit": opt.commit, "what": "wall time of one %d-step rollout, %d alternating repetitions after %d warm-up "
                                         "rollouts each" % (T, opt.reps, opt.warmup),
           "eager": e, "graph": g, "spread_ms": round(spread, 4),
           "spread_is": "the larger of the two ways' 10th-to-90th-percentile widths",
           "graph_faster_by_ms": round(e["median_ms"] - g["median_ms"], 4),
           "graph_is_default": bool(e["median_ms"] - g["median_ms"] > spread),
           "eager_ms_per_env_step": round(e["median_ms"] / T, 4), "graph_ms_per_env_step": round(g["median_ms"] / T, 4),
           "eager_launches_per_step": None, "eager_device_activities_per_step": None,
           "eager_launches_note": "not counted",
           "graph_launches_per_step": "1 graph launch + %d slab writes (+ the integer actions' conversion per agent)"
                                      % len(runner.buffer)}

    kept = open(opt.out).read() if opt.out and opt.append and os.path.exists(opt.out) else ""

    def write():
        if opt.out:
            os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
            with open(opt.out, "w") as f:
                f.write(kept + json.dumps(out) + "\n")
    write()                                 # (the timings are on disk before the profiler starts)
    try:                                    # in a run of its own: tracing slows the host
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for step in range(4):
                eager_step(step)
            torch.cuda.synchronize()
        device = [ev for ev in prof.events() if str(ev.device_type).endswith("CUDA")]
        kernels = [ev for ev in device if not ev.name.lower().startswith(("memcpy", "memset"))]
        if kernels:
            launches, activities = len(kernels) / 4.0, len(device) / 4.0
        else:
            why = "the profiler recorded no kernel"
    except Exception as exc:
        why = "%s: %s" % (type(exc).__name__, exc)

    out["eager_launches_per_step"], out["eager_device_activities_per_step"] = launches, activities
    out["eager_launches_note"] = why
    write()
    print(json.dumps(out))
