#!/usr/bin/env python
"""Steps device-resident simple_push worlds through their kernel path (``mappo_simple_push_step``, one launch per step)
-- or, with ``--scenario simple_tag --num_adversaries V``, simple_tag worlds through ``mappo_simple_tag_step``, or, with
``--scenario simple_world_comm --num_adversaries V``, simple_world_comm worlds (``--num_landmarks`` obstacles) through
``mappo_simple_world_comm_step`` -- and nothing else, for a kernel-trace run of its own:

    rocprofv3 --kernel-trace --stats -f csv -d out -o push -- python tools/push_step_trace.py --worlds 4096

The trace's ``push_step_kernel`` (``tag_step_kernel``, ``world_comm_step_kernel``) row is the step kernel's own time at that number of worlds (the generator draws of a
step and the action tensor are separate kernels in the same trace).  Prints one JSON line with the shape and the wall
time per step as the host sees it.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "on-policy_amd"))

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenario", default="simple_push", choices=("simple_push", "simple_tag", "simple_world_comm"))
    ap.add_argument("--num_adversaries", type=int, default=3, help="simple_tag / simple_world_comm only: of --num_agents")
    ap.add_argument("--worlds", type=int, default=128)
    ap.add_argument("--num_agents", type=int, default=2)
    ap.add_argument("--num_landmarks", type=int, default=2)
    ap.add_argument("--steps", type=int, default=200)
    opt = ap.parse_args()
    import torch
    from onpolicy.envs.mpe.simple_push import TorchSimplePush
    from onpolicy.envs.mpe.simple_tag import TorchSimpleTag
    from onpolicy.envs.mpe.simple_world_comm import TorchSimpleWorldComm
    assert torch.cuda.is_available(), "a trace needs the GPU"
    dev = torch.device("cuda", 0)
    if opt.scenario in ("simple_tag", "simple_world_comm"):
        cls = TorchSimpleTag if opt.scenario == "simple_tag" else TorchSimpleWorldComm
        env = cls(opt.worlds, opt.num_agents, opt.num_landmarks, seed=1, device=dev, num_adversaries=opt.num_adversaries)
    else:
        env = TorchSimplePush(opt.worlds, opt.num_agents, opt.num_landmarks, seed=1, device=dev)
    assert env.graph_safe
    env.reset()
    g = torch.Generator(device=dev).manual_seed(2)
    actions = [torch.randint(0, 5, (opt.worlds, opt.num_agents), generator=g, device=dev) for _ in range(8)]
    if opt.scenario == "simple_world_comm":     # the leader's word goes between its movement and the others'
        actions = [torch.cat([a[:, :1], torch.randint(0, 4, (opt.worlds, 1), generator=g, device=dev), a[:, 1:]], 1)
                   for a in actions]
    for i in range(10):
        env.step(actions[i % 8])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(opt.steps):
        env.step(actions[i % 8])
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    print(json.dumps({"scenario": opt.scenario, "worlds": opt.worlds, "num_agents": opt.num_agents,
                      "num_landmarks": opt.num_landmarks, "steps": opt.steps,
                      "host_us_per_step": round(1e6 * wall / opt.steps, 2)}))
