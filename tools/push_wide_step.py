#!/usr/bin/env python
"""The simple_push step kernel of K11 wide (``mappo_simple_push_step_wide``), measured on one MI355X: against the thin
kernel (``mappo_simple_push_step``) at the shapes both take, against the tensor-op step (``_step_ops``) that serves the
larger shapes without it.

    python tools/push_wide_step.py --out profiles/push_wide_step.json

Timing: a step kernel alone is ``--inner`` launches on preallocated operands (one set of restart draws, the outputs
overwritten), captured once into a graph -- a plain chain -- and replayed between device events, so that no host time
lies between the launches; a tensor-op step is the eager ``_step_ops`` with its generator draws, ``--inner`` of them
between device events, as a rollout without the kernel pays for it.  Per shape (agents, landmarks) and number of worlds,
``--reps`` repetitions of each path, alternating.  Medians and 10th-to-90th-percentile widths per step.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "on-policy_amd"))
COPY_CEILING = 6.29e12      # bytes/s, the float4 copy the project quotes as the MI355X's streaming ceiling
BOTH = ((2, 2), (3, 2), (16, 2))        # thin against wide
WIDE_ONLY = ((32, 2), (64, 2))          # wide against the tensor-op step
WORLDS = (128, 4096)


def spread(xs):
    q = statistics.quantiles(xs, n=10)
    return q[-1] - q[0]


def between_events(torch, run, inner):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    run()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / inner


def kernel_chain(torch, env, actions, inner):
    """-> a callable that replays ``inner`` launches of env's step kernel and nothing else."""
    dev = env.device
    idx = env._kernel_actions(actions).to(torch.int64).contiguous()
    fresh = env._fresh()
    obs = torch.empty(env._obs_shape(), dtype=torch.float32, device=dev)
    rewards = torch.empty(env.n, env.a, 1, dtype=torch.float32, device=dev)
    dones = torch.empty(env.n, env.a, dtype=torch.bool, device=dev)
    per_agent = torch.empty(env.n, env.a, dtype=torch.float64, device=dev)
    launch = lambda: env._launch(idx, fresh, obs, rewards, dones, per_agent)      # noqa: E731
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        launch()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(inner):
            launch()
    return lambda keep=(idx, fresh, obs, rewards, dones, per_agent): graph.replay()      # (the operands live as long)


def timings(opt):
    import torch
    from onpolicy.envs.mpe.simple_push import TorchSimplePush
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda", 0)
    out = {}
    for agents, landmarks in BOTH + WIDE_ONLY:
        for worlds in WORLDS:
            wide, other = (TorchSimplePush(worlds, agents, landmarks, seed=1, device=dev, wide=w) for w in (True, False))
            assert wide.graph_safe and wide._wide and other.graph_safe == ((agents, landmarks) in BOTH)
            wide.reset(), other.reset()
            g = torch.Generator(device=dev).manual_seed(2)
            actions = [torch.randint(0, 5, (worlds, agents), generator=g, device=dev) for _ in range(8)]
            paths = {"wide_kernel": kernel_chain(torch, wide, actions[0], opt.inner)}
            if other.graph_safe:
                against = "thin_kernel"
                paths[against] = kernel_chain(torch, other, actions[0], opt.inner)
            else:
                against = "tensor_ops"
                paths[against] = lambda: [other._step_ops(actions[i % 8]) for i in range(opt.inner)]
            for run in paths.values():
                between_events(torch, run, opt.inner)
            us = {name: [] for name in paths}
            for _ in range(opt.reps):
                for name, run in paths.items():
                    us[name].append(1e3 * between_events(torch, run, opt.inner))
            row = {"agents": agents, "landmarks": landmarks, "worlds": worlds}
            for name, xs in us.items():
                row[name + "_median_us"] = round(statistics.median(xs), 2)
                row[name + "_spread_us"] = round(spread(xs), 2)
            gain = row[against + "_median_us"] - row["wide_kernel_median_us"]
            row["wide_wins_by_more_than_the_spread"] = bool(
                gain > max(row[against + "_spread_us"], row["wide_kernel_spread_us"]))
            row["obs_bytes_per_step"] = 4 * worlds * sum(wide.obs_dims)
            row["obs_write_TBps"] = round(row["obs_bytes_per_step"] / (row["wide_kernel_median_us"] * 1e-6) / 1e12, 3)
            row["of_copy_ceiling"] = round(row["obs_write_TBps"] * 1e12 / COPY_CEILING, 3)
            out["a%dl%dx%d" % (agents, landmarks, worlds)] = row
            print(json.dumps(row), flush=True)
            del wide, other, paths
            torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--out", required=True)
    opt = ap.parse_args()
    result = {"what": "simple_push through K11 wide on one MI355X (tools/push_wide_step.py): the step kernel alone (%d "
                      "launches on preallocated operands, replayed from one captured chain between device events) at "
                      "(agents, landmarks) = (2, 2), (3, 2) and (16, 2) against the thin kernel measured the same way, "
                      "at (32, 2) and (64, 2) against the eager tensor-op step with its generator draws; medians of %d "
                      "alternating repetitions, spread = 10th-to-90th-percentile width; the observation bytes a step "
                      "writes over the wide kernel's time next to the 6.29 TB/s copy ceiling" % (opt.inner, opt.reps),
              "step_kernel": timings(opt)}
    with open(opt.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", opt.out)
