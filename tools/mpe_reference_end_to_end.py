#!/usr/bin/env python
"""The reference's train_mpe_reference.sh (MPE simple_reference, 2 agents, 3 landmarks, rmappo, episode_length 25,
ppo_epoch 15, num_mini_batch 1, gain 0.01, lr / critic_lr 7e-4) at n_rollout_threads=4096 on one MI355X, worlds resident
on the device (--use_device_env): rollout (policy forward -> MultiDiscrete sampling (K14) -> simple_reference step
(K11 family) -> K2 insert) AND update (compute_returns + R_MAPPO.train) through the unmodified train script / runner.

    python tools/mpe_reference_end_to_end.py [--threads 4096] [--iterations 3] [--commit HASH] [--out file.json]

Prints one JSON line: env-steps/s of a whole iteration (rollout + update) in steady state, the rollout phase alone,
and whether the rollout ran from the captured graph.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "on-policy_amd"))

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=4096)
    ap.add_argument("--episode_length", type=int, default=25)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--algorithm_name", default="rmappo")
    ap.add_argument("--commit", default=None, help="commit the measurement was made on (recorded in the JSON line)")
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    os.environ.setdefault("MAPPO_RESULTS_DIR", tempfile.mkdtemp())
    import torch
    from onpolicy.scripts.train import train_mpe
    T, N = opt.episode_length, opt.threads
    argv = ["--env_name", "MPE", "--algorithm_name", opt.algorithm_name, "--experiment_name", "check",
            "--scenario_name", "simple_reference", "--num_agents", "2", "--num_landmarks", "3", "--seed", "1",
            "--n_training_threads", "1", "--n_rollout_threads", str(N), "--num_mini_batch", "1",
            "--episode_length", str(T), "--num_env_steps", str(T * N), "--ppo_epoch", "15", "--gain", "0.01",
            "--lr", "7e-4", "--critic_lr", "7e-4", "--use_wandb", "--log_interval", "1000", "--save_interval", "1000",
            "--use_device_env"]
    t0 = time.time()
    runner = train_mpe.main(argv)           # one whole iteration: builds everything, warms allocator and kernels
    torch.cuda.synchronize()
    first = time.time() - t0
    graphed = getattr(runner, "rollout_graph", None) is not None

    def rollout():
        if graphed:
            runner.trainer.prep_rollout()
            runner.rollout_graph.begin_episode()
            for step in range(T):
                runner.rollout_graph.step()
            return
        for step in range(T):
            values, actions, action_log_probs, rnn_states, rnn_states_critic, actions_env = runner.collect(step)
            obs, rewards, dones, infos = runner.envs.step(actions_env)
            runner.insert((obs, rewards, dones, infos, values, actions, action_log_probs, rnn_states, rnn_states_critic))

    roll, upd = [], []
    for _ in range(opt.iterations):
        torch.cuda.synchronize()
        a = time.perf_counter()
        rollout()
        torch.cuda.synchronize()
        b = time.perf_counter()
        runner.compute()
        info = runner.train()
        torch.cuda.synchronize()
        c = time.perf_counter()
        roll.append(b - a)
        upd.append(c - b)
    r, u = sum(roll) / len(roll), sum(upd) / len(upd)
    out = {"config": "train_mpe_reference.sh: MPE simple_reference, 2 agents, 3 landmarks, %s, n_rollout_threads=%d, "
                     "episode_length=%d, ppo_epoch=15, 1 x MI355X, worlds on the device" % (opt.algorithm_name, N, T),
           "commit": opt.commit,
           "rollout_graph": "yes" if graphed else "no",
           "env_steps_per_s_rollout_plus_update": round(T * N / (r + u), 1),
           "rollout_env_steps_per_s": round(T * N / r, 1),
           "rollout_s": round(r, 4), "rollout_ms_per_env_step": round(1e3 * r / T, 4),
           "update_s": round(u, 4),
           "iterations": opt.iterations, "first_iteration_incl_startup_s": round(first, 2),
           "mean_reward_last_rollout": float(runner.buffer.rewards.mean()),
           "train_info": {k: round(float(v), 6) for k, v in info.items()}}
    line = json.dumps(out)
    print(line)
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as f:
            f.write(line + "\n")
