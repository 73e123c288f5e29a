#!/usr/bin/env python
"""The simple_spread step past 16 entities, measured on one MI355X: K11 wide (``mappo_simple_spread_step_wide``) against
the tensor-op step (``_step_ops``) that served these shapes before it, and the step kernels' own times from traces.

    python tools/spread_wide_step.py [--traces DIR] --out profiles/spread_wide_step.json

Timing: per shape (agents = landmarks) and number of worlds, ``--reps`` repetitions of ``--inner`` steps of each path,
alternating, between device events; both paths make the step's generator draws and allocate its outputs, as a rollout
pays for them.  Medians and 10th-to-90th-percentile widths per step.  ``--traces DIR``: DIR/<label>/ holds one
``rocprofv3 --kernel-trace`` run of ``tools/push_step_trace.py --scenario simple_spread`` each (label =
<agents>x<worlds>, with a leading ``wide_`` for a run under MAPPO_SPREAD_WIDE=1); the median over the launches of each
step kernel found there is recorded, with the observation bytes per step over that time where the wide kernel ran.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "on-policy_amd"))
COPY_CEILING = 6.29e12      # bytes/s, the float4 copy the project quotes as the MI355X's streaming ceiling


def spread(xs):
    q = statistics.quantiles(xs, n=10)
    return q[-1] - q[0]


def obs_bytes(agents, landmarks, worlds):
    return 4 * worlds * agents * (4 + 2 * landmarks + 4 * (agents - 1))


def traces(root):
    out = {}
    for d in sorted(glob.glob(os.path.join(root, "*x*", ""))):
        d = d.rstrip(os.sep)
        label = os.path.basename(d)
        agents, worlds = (int(x) for x in label.replace("wide_", "").split("x"))
        durations = {}
        for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                if "spread_step" in r["Kernel_Name"]:
                    name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].strip()
                    durations.setdefault(name, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
        for name, ns in durations.items():
            row = {"kernel": name, "agents": agents, "landmarks": agents, "worlds": worlds, "launches": len(ns),
                   "median_us": round(statistics.median(ns) / 1e3, 2), "spread_us": round(spread(ns) / 1e3, 2)}
            if "wide" in name:
                row["obs_bytes_per_step"] = obs_bytes(agents, agents, worlds)
                row["obs_write_TBps"] = round(row["obs_bytes_per_step"] / (statistics.median(ns) * 1e-9) / 1e12, 3)
                row["of_copy_ceiling"] = round(row["obs_write_TBps"] * 1e12 / COPY_CEILING, 3)
            out[label] = row
    return out


def time_steps(torch, step, actions, inner):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(inner):
        step(actions[i % len(actions)])
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / inner


def timings(opt):
    import torch
    from onpolicy.envs.mpe.simple_spread import TorchSimpleSpread
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda", 0)
    out = {}
    for agents in (32, 64):
        for worlds in (128, 4096):
            kernel = TorchSimpleSpread(worlds, agents, agents, seed=1, device=dev)
            tensor = TorchSimpleSpread(worlds, agents, agents, seed=1, device=dev)
            assert kernel.graph_safe and kernel._wide
            kernel.reset(), tensor.reset()
            g = torch.Generator(device=dev).manual_seed(2)
            actions = [torch.randint(0, 5, (worlds, agents), generator=g, device=dev) for _ in range(8)]
            paths = {"wide_kernel": kernel.step, "tensor_ops": tensor._step_ops}
            for step in paths.values():
                time_steps(torch, step, actions, 3)
            ms = {name: [] for name in paths}
            for _ in range(opt.reps):
                for name, step in paths.items():
                    ms[name].append(time_steps(torch, step, actions, opt.inner))
            row = {"agents": agents, "landmarks": agents, "worlds": worlds}
            for name, xs in ms.items():
                row[name + "_median_ms"] = round(statistics.median(xs), 4)
                row[name + "_spread_ms"] = round(spread(xs), 4)
            gain = row["tensor_ops_median_ms"] - row["wide_kernel_median_ms"]
            row["kernel_wins_by_more_than_the_spread"] = bool(
                gain > max(row["tensor_ops_spread_ms"], row["wide_kernel_spread_ms"]))
            out["%dx%d" % (agents, worlds)] = row
            print(json.dumps(row), flush=True)
            del kernel, tensor
            torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--traces", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", required=True)
    opt = ap.parse_args()
    result = {"what": "simple_spread past 16 entities on one MI355X (tools/spread_wide_step.py): `step_time` = a whole env "
                      "step (generator draws, output allocation, the step) through K11 wide and as tensor operations, "
                      "medians of %d alternating repetitions of %d steps between device events, spread = "
                      "10th-to-90th-percentile width; `kernel_trace` = the step kernel's own time, median over the "
                      "launches of one rocprofv3 --kernel-trace run of tools/push_step_trace.py --scenario simple_spread "
                      "per shape (labels agents x worlds, landmarks = agents; wide_ = MAPPO_SPREAD_WIDE=1), with the "
                      "observation bytes a step writes over that time next to the 6.29 TB/s copy ceiling"
                      % (opt.reps, opt.inner),
              "step_time": timings(opt)}
    if opt.traces:
        result["kernel_trace"] = traces(opt.traces)
    with open(opt.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", opt.out)
