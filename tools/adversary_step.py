#!/usr/bin/env python
"""The simple_adversary step kernel (``mappo_simple_adversary_step``) alone, measured on one MI355X.

    python tools/adversary_step.py --out profiles/adversary_step.json

Per shape (agents x worlds; A - 1 landmarks): ``--reps`` repetitions of ``--inner`` launches back to back on one stream
between device events, on operands allocated and drawn once (the launch alone: no generator draws, no allocation), after
``--warmup`` untimed launches.  ``us_per_launch`` is the median over the repetitions of the window over ``--inner``: the
kernel's time plus whatever gap the stream leaves between two launches, so an upper bound of the kernel time, and at the
small shapes mostly that gap.  ``spread_us`` is the 10th-to-90th-percentile width.  ``bytes_per_step`` counts what the
algorithm has to move -- state read and written, actions, outputs -- from the shapes; ``obs_write_TBps`` is the observation
bytes alone over that time, next to the 6.29 TB/s float4 copy the project quotes as the MI355X's streaming ceiling.
Recorded, not tuned.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "on-policy_amd"))
COPY_CEILING = 6.29e12      # bytes/s
SHAPES = ((3, 128), (3, 4096), (64, 128), (64, 4096))


def step_bytes(a, l, n):
    """-> (observation bytes, all bytes) one step of n worlds reads and writes."""
    from onpolicy.envs.mpe.simple_adversary import obs_widths
    obs = 4 * n * sum(obs_widths(a, l))
    state = n * (2 * 2 * a * 16 + l * 16 + 2 * 8 + 8)       # pos / vel in and out, landmarks, t in and out, goal
    return obs, obs + state + n * a * (8 + 4 + 1 + 8)       # + actions, rewards, dones, per_agent


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", required=True)
    opt = ap.parse_args()
    import torch
    from onpolicy.envs.mpe.simple_adversary import TorchSimpleAdversary
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda", 0)
    rows = {}
    for a, n in SHAPES:
        env = TorchSimpleAdversary(n, a, seed=1, device=dev)
        env.reset()
        act = torch.randint(0, 5, (n, a), device=dev)
        fresh = env._fresh()
        obs = torch.empty(env._obs_shape(), dtype=torch.float32, device=dev)
        rew = torch.empty(n, a, 1, dtype=torch.float32, device=dev)
        dones = torch.empty(n, a, dtype=torch.bool, device=dev)
        per_agent = torch.empty(n, a, dtype=torch.float64, device=dev)
        launch = lambda: env._launch(act, fresh, obs, rew, dones, per_agent)      # noqa: E731
        for _ in range(opt.warmup):
            launch()
        us = []
        for _ in range(opt.reps):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(opt.inner):
                launch()
            stop.record()
            stop.synchronize()
            us.append(1e3 * start.elapsed_time(stop) / opt.inner)
        assert bool(torch.isfinite(obs).all())
        q = statistics.quantiles(us, n=10)
        med = statistics.median(us)
        obs_b, all_b = step_bytes(a, a - 1, n)
        rows["%dx%d" % (a, n)] = {
            "agents": a, "landmarks": a - 1, "worlds": n, "lanes_per_world": 32 if a <= 32 else 64,
            "us_per_launch": round(med, 2), "spread_us": round(q[-1] - q[0], 2), "obs_bytes_per_step": obs_b,
            "bytes_per_step": all_b, "obs_write_TBps": round(obs_b / (med * 1e-6) / 1e12, 4),
            "of_copy_ceiling": round(obs_b / (med * 1e-6) / COPY_CEILING, 4)}
        print(json.dumps(rows["%dx%d" % (a, n)]), flush=True)
        del env, obs
        torch.cuda.empty_cache()
    out = {"what": "mappo_simple_adversary_step alone on one MI355X (tools/adversary_step.py): median over %d repetitions "
                   "of the time of %d back-to-back launches between device events, per launch (kernel time plus the "
                   "stream's gap between launches: an upper bound of the kernel time), spread = 10th-to-90th-percentile "
                   "width; the observation bytes a step writes over that time next to the 6.29 TB/s copy ceiling"
                   % (opt.reps, opt.inner),
           "commit": opt.commit, "shapes": rows}
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", opt.out)
