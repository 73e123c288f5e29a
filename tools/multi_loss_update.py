#!/usr/bin/env python
"""One ``R_MAPPO.train()`` of the reference's train_mpe_reference.sh (MPE simple_reference, 2 agents, 3 landmarks, rmappo,
128 rollout threads, 25 steps, hidden 64, 15 epochs of one minibatch = 6,400 rows) on one MI355X, timed two ways in the
same process, alternating: the default route for its MultiDiscrete (5, 10) head -- the framework loss, eager updates --
and the opt-in route (MAPPO_FUSED_LOSS_MULTI=1 / --fused_multi_loss: ``mappo_ppo_loss_multi_f32`` + the captured update).
Both trainers start from the same weights and train on the same rollout; each keeps its own policy.

    python tools/multi_loss_update.py [--reps 30] [--warmup 3] [--commit HASH] [--out file.json]

Per way: median, quartiles, 10th / 90th percentile and range of the wall time of one train() (host clock around work that
ends in a device synchronise) over ``--reps`` calls after ``--warmup`` untimed ones (the opt-in route's warm-up holds its
eager update and its capture).  ``spread_ms`` is the larger of the two 10th-to-90th-percentile widths; the opt-in route is
faster only if its median is below the default's by more than that.  ``launches_per_update``: kernels of one train()
divided by its 15 updates, counted by the framework's profiler in a run of its own after the timing (a graph replay's
kernels are counted as the device ran them; null with the reason where the profiler is not available).  Prints one JSON line.
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
    ap.add_argument("--threads", type=int, default=128)
    ap.add_argument("--episode_length", type=int, default=25)
    ap.add_argument("--hidden_size", type=int, default=64)
    ap.add_argument("--ppo_epoch", type=int, default=15)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--commit", default=None, help="commit the measurement was made on (recorded in the JSON line)")
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    os.environ.setdefault("MAPPO_RESULTS_DIR", tempfile.mkdtemp())
    os.environ.pop("MAPPO_FUSED_LOSS_MULTI", None)
    import copy
    import torch
    from onpolicy.algorithms.r_mappo.algorithm.rMAPPOPolicy import R_MAPPOPolicy
    from onpolicy.algorithms.r_mappo.r_mappo import R_MAPPO
    from onpolicy.scripts.train import train_mpe
    assert torch.cuda.is_available(), "a timing needs the GPU"
    T, N = opt.episode_length, opt.threads
    argv = ["--env_name", "MPE", "--algorithm_name", "rmappo", "--experiment_name", "check",
            "--scenario_name", "simple_reference", "--num_agents", "2", "--num_landmarks", "3", "--seed", "1",
            "--n_training_threads", "1", "--n_rollout_threads", str(N), "--num_mini_batch", "1",
            "--episode_length", str(T), "--num_env_steps", str(T * N), "--ppo_epoch", str(opt.ppo_epoch), "--gain", "0.01",
            "--lr", "7e-4", "--critic_lr", "7e-4", "--hidden_size", str(opt.hidden_size), "--use_wandb",
            "--log_interval", "1000", "--save_interval", "1000", "--use_device_env"]
    runner = train_mpe.main(argv)           # one whole iteration: worlds, one rollout in the buffer, one train()
    args, buf, dev = runner.all_args, runner.buffer, runner.device
    spaces = (runner.envs.observation_space[0],
              runner.envs.share_observation_space[0] if runner.use_centralized_V else runner.envs.observation_space[0],
              runner.envs.action_space[0])

    def make(opt_in):
        a = copy.copy(args)
        a.fused_multi_loss = opt_in
        policy = R_MAPPOPolicy(a, *spaces, device=dev)
        policy.actor.load_state_dict(runner.policy.actor.state_dict())
        policy.critic.load_state_dict(runner.policy.critic.state_dict())
        trainer = R_MAPPO(a, policy, device=dev)
        assert trainer._fused_loss is opt_in
        trainer.prep_training()
        return trainer

    trainers = {"default": make(False), "opt_in": make(True)}
    buf.compute_returns(torch.zeros(buf.value_preds.shape[1:], device=dev), trainers["default"].value_normalizer)

    def timed(trainer):
        torch.cuda.synchronize()
        a = time.perf_counter()
        trainer.train(buf)                  # (ends in the one device -> host read of the logged means)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - a)

    for _ in range(opt.warmup):
        for tr in trainers.values():
            timed(tr)
    times = {k: [] for k in trainers}
    for _ in range(opt.reps):               # alternating: both ways see the same machine
        for k, tr in trainers.items():
            times[k].append(timed(tr))
    d, o = summary(times["default"]), summary(times["opt_in"])
    spread = max(d["p90_ms"] - d["p10_ms"], o["p90_ms"] - o["p10_ms"])
    ug = trainers["opt_in"]._update_graph
    out = {"config": "train_mpe_reference.sh: MPE simple_reference, 2 agents, 3 landmarks, rmappo, n_rollout_threads=%d, "
                     "episode_length=%d, hidden_size=%d, ppo_epoch=%d, num_mini_batch=1 (%d rows per update), 1 x MI355X"
                     % (N, T, opt.hidden_size, opt.ppo_epoch, N * T * 2),
           "commit": opt.commit, "what": "wall time of one train(), %d alternating repetitions after %d warm-up calls each"
                                         % (opt.reps, opt.warmup),
           "default": d, "opt_in": o, "spread_ms": round(spread, 4),
           "spread_is": "the larger of the two ways' 10th-to-90th-percentile widths",
           "opt_in_faster_by_ms": round(d["median_ms"] - o["median_ms"], 4),
           "opt_in_is_faster_beyond_the_spread": bool(d["median_ms"] - o["median_ms"] > spread),
           "default_ms_per_update": round(d["median_ms"] / opt.ppo_epoch, 4),
           "opt_in_ms_per_update": round(o["median_ms"] / opt.ppo_epoch, 4),
           "opt_in_update_graph": {"captures": ug.captures, "warmups": ug.warmups, "replays": ug.replays,
                                   "capture_failures": ug.capture_failures},
           "launches_per_update": {"default": None, "opt_in": None}, "launches_note": "not counted"}

    def write():
        if opt.out:
            os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
            with open(opt.out, "w") as f:
                f.write(json.dumps(out) + "\n")
    write()                                 # (the timings are on disk before the profiler starts)
    why = None
    try:                                    # in a run of its own: tracing slows the host
        from torch.profiler import ProfilerActivity, profile
        for k, tr in trainers.items():
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                tr.train(buf)
                torch.cuda.synchronize()
            device = [ev for ev in prof.events() if str(ev.device_type).endswith("CUDA")]
            kernels = [ev for ev in device if not ev.name.lower().startswith(("memcpy", "memset"))]
            if kernels:
                out["launches_per_update"][k] = round(len(kernels) / float(opt.ppo_epoch), 1)
            else:
                why = "the profiler recorded no kernel"
    except Exception as exc:
        why = "%s: %s" % (type(exc).__name__, exc)
    out["launches_note"] = why
    write()
    print(json.dumps(out))
