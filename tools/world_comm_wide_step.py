#!/usr/bin/env python
"""The simple_world_comm step through K11 wide (``mappo_simple_world_comm_step_wide``), measured on one MI355X: against
the thin kernel (``mappo_simple_world_comm_step``) at the script's shape, which both take, against the tensor-op step
(``_step_ops``) that serves the larger shapes without it, and the step kernels' own times from traces.

    python tools/world_comm_wide_step.py [--traces DIR] --out profiles/world_comm_wide_step.json

Timing: per shape (adversaries, good agents, obstacles) at ``--worlds`` worlds, ``--reps`` repetitions of ``--inner``
steps of each path, alternating, between device events; every path makes the step's generator draws and allocates its
outputs, as a rollout pays for them.  Medians and 10th-to-90th-percentile widths per step.  ``--traces DIR``:
DIR/<label>/ holds one ``rocprofv3 --kernel-trace`` run of ``tools/push_step_trace.py --scenario simple_world_comm``
each (label = <adversaries>v<good>l<obstacles>x<worlds>, with a leading ``wide_`` for a run under
MAPPO_WORLD_COMM_WIDE=1); the median over the launches of each step kernel found there is recorded, with the observation
bytes per step over that time where the wide kernel ran.
"""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "on-policy_amd"))
COPY_CEILING = 6.29e12      # bytes/s, the float4 copy the project quotes as the MI355X's streaming ceiling
BOTH = ((4, 2, 1),)                     # thin against wide
WIDE_ONLY = ((13, 4, 2), (48, 16, 60))  # wide against the tensor-op step


def spread(xs):
    q = statistics.quantiles(xs, n=10)
    return q[-1] - q[0]


def obs_bytes(adv, good, obstacles, worlds):
    from onpolicy.envs.mpe.simple_world_comm import obs_widths
    return 4 * worlds * sum(obs_widths(adv, good, obstacles))


def traces(root):
    out = {}
    for d in sorted(glob.glob(os.path.join(root, "*v*l*x*", ""))):
        label = os.path.basename(d.rstrip(os.sep))
        adv, good, obstacles, worlds = (int(x) for x in re.match(r"(?:wide_)?(\d+)v(\d+)l(\d+)x(\d+)$", label).groups())
        durations = {}
        for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                if "world_comm_step" in r["Kernel_Name"]:
                    name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].strip()
                    durations.setdefault(name, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
        for name, ns in durations.items():
            row = {"kernel": name, "adversaries": adv, "good": good, "obstacles": obstacles, "worlds": worlds,
                   "launches": len(ns), "median_us": round(statistics.median(ns) / 1e3, 2),
                   "spread_us": round(spread(ns) / 1e3, 2)}
            if "wide" in name:
                row["obs_bytes_per_step"] = obs_bytes(adv, good, obstacles, worlds)
                row["obs_write_TBps"] = round(row["obs_bytes_per_step"] / (statistics.median(ns) * 1e-9) / 1e12, 3)
                row["of_copy_ceiling"] = round(row["obs_write_TBps"] * 1e12 / COPY_CEILING, 3)
            out[label] = row
    if "4v2l1x4096" in out and "wide_4v2l1x4096" in out:
        thin, wide = out["4v2l1x4096"], out["wide_4v2l1x4096"]
        wide["beats_the_thin_kernel_by_more_than_the_spread"] = bool(
            thin["median_us"] - wide["median_us"] > max(thin["spread_us"], wide["spread_us"]))
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
    from onpolicy.envs.mpe.simple_world_comm import TorchSimpleWorldComm
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda", 0)
    out, worlds = {}, opt.worlds
    for adv, good, obstacles in BOTH + WIDE_ONLY:
        agents = adv + good
        wide, other = (TorchSimpleWorldComm(worlds, agents, obstacles, seed=1, device=dev, num_adversaries=adv, wide=w)
                       for w in (True, False))
        assert wide.graph_safe and wide._wide and other.graph_safe == ((adv, good, obstacles) in BOTH)
        wide.reset(), other.reset()
        g = torch.Generator(device=dev).manual_seed(2)
        draw = lambda high, cols: torch.randint(0, high, (worlds, cols), generator=g, device=dev)      # noqa: E731
        actions = [torch.cat([draw(5, 1), draw(4, 1), draw(5, agents - 1)], 1) for _ in range(8)]
        against = "thin_kernel" if other.graph_safe else "tensor_ops"
        paths = {"wide_kernel": wide.step, against: other.step}      # (step takes the tensor path past the thin caps)
        for step in paths.values():
            time_steps(torch, step, actions, 3)
        ms = {name: [] for name in paths}
        for _ in range(opt.reps):
            for name, step in paths.items():
                ms[name].append(time_steps(torch, step, actions, opt.inner))
        row = {"adversaries": adv, "good": good, "obstacles": obstacles, "worlds": worlds}
        for name, xs in ms.items():
            row[name + "_median_ms"] = round(statistics.median(xs), 4)
            row[name + "_spread_ms"] = round(spread(xs), 4)
        gain = row[against + "_median_ms"] - row["wide_kernel_median_ms"]
        row["wide_wins_by_more_than_the_spread"] = bool(
            gain > max(row[against + "_spread_ms"], row["wide_kernel_spread_ms"]))
        out["%dv%dl%dx%d" % (adv, good, obstacles, worlds)] = row
        print(json.dumps(row), flush=True)
        del wide, other
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--traces", default=None)
    ap.add_argument("--worlds", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--out", required=True)
    opt = ap.parse_args()
    result = {"what": "simple_world_comm through K11 wide on one MI355X (tools/world_comm_wide_step.py): `step_time` = a "
                      "whole env step (generator draws, output allocation, the step) of %d worlds through the wide kernel "
                      "and, at (4, 2, 1), through the thin kernel, at (13, 4, 2) and (48, 16, 60) as tensor operations, "
                      "medians of %d alternating repetitions of %d steps between device events, spread = "
                      "10th-to-90th-percentile width; `kernel_trace` = the step kernel's own time, median over the "
                      "launches of one rocprofv3 --kernel-trace run of tools/push_step_trace.py --scenario "
                      "simple_world_comm per shape (labels adversaries v good l obstacles x worlds; wide_ = "
                      "MAPPO_WORLD_COMM_WIDE=1), with the observation bytes a step writes over that time next to the "
                      "6.29 TB/s copy ceiling" % (opt.worlds, opt.reps, opt.inner),
              "step_time": timings(opt)}
    if opt.traces:
        result["kernel_trace"] = traces(opt.traces)
    with open(opt.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", opt.out)
