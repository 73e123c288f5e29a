#!/usr/bin/env python
"""Are two builds of libmappo_hip.so the SAME function on the device MPE envs and the rollout samplers, and as fast?

bits    simple_spread (3 and 16 agents) and simple_reference, 4096 worlds, 300 steps each on seeded actions across several
        auto-resets (episode length 25); K14 (8192 x 5 and 4096 x 48, with and without an availability mask) and its
        MultiDiscrete form (8192 rows, heads [5, 10] and [3, 7, 2]) on seeded logits.  Once per library in two fresh child
        processes; every output and state tensor must be bit-identical (np.array_equal).
time    per-launch time of spread_step_kernel (4096 worlds, 3 agents), reference_step_kernel (4096 worlds),
        categorical_sample_kernel (8192 x 5) and multi_categorical_sample_kernel (8192 rows, heads [5, 10]) from
        rocprofv3 --kernel-trace --stats, old and new library alternating, --pairs times; and, with --bench-pairs, ms_per_step
        of the plain north-star bench line, alternating likewise.  A kernel passes when the new library's median lies within
        the old library's own min-max range over the pairs.

    tools/ab_old_lib.sh                     # the parent commit's library -> on-policy_amd/lib/libmappo_hip_OLD.so
    python tools/ab_mpe_core.py --old on-policy_amd/lib/libmappo_hip_OLD.so [--pairs 5] [--bench-pairs 3] [--json OUT.json]
Exit status 0: identical and within the old library's spread; 1 otherwise.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("spread_step_kernel", "reference_step_kernel", "multi_categorical_sample_kernel", "categorical_sample_kernel")
WORLDS, STEPS, LAUNCHES = 4096, 300, 200


def _setup():
    sys.path.insert(0, os.path.join(ROOT, "on-policy_amd"))
    import torch
    from onpolicy.algorithms.utils import fused_loss
    from onpolicy.envs.mpe.simple_reference import TorchSimpleReference
    from onpolicy.envs.mpe.simple_spread import TorchSimpleSpread
    return torch, fused_loss, TorchSimpleSpread, TorchSimpleReference


def _actions(torch, env, gen):
    if hasattr(env, "goal"):        # (movement, symbol)
        return torch.stack([torch.randint(0, 5, (env.n, env.a), generator=gen), torch.randint(0, 10, (env.n, env.a), generator=gen)],
                           -1).cuda()
    return torch.randint(0, 5, (env.n, env.a, 1), generator=gen).cuda()


def child_bits(outdir):
    import numpy as np
    torch, fused_loss, Spread, Reference = _setup()
    from onpolicy import _native
    arrays = {}
    envs = {"spread3": Spread(WORLDS, 3, device="cuda", seed=11), "spread16": Spread(WORLDS, 16, device="cuda", seed=12),
            "reference": Reference(WORLDS, device="cuda", seed=13)}
    for name, env in envs.items():
        assert env.graph_safe
        gen = torch.Generator().manual_seed(5)
        arrays[name + ".obs0"] = env.reset()
        acc = None
        for step in range(STEPS):
            out = env.step(_actions(torch, env, gen))
            # every step's outputs enter an exact running sum in float64 (obs / rewards / per-agent) and the dones a count;
            # the last step's are kept whole as well
            cur = [out[0].double(), out[1].double(), out[2].long(), out[3]._per_agent.clone()]
            acc = cur if acc is None else [a + c for a, c in zip(acc, cur)]
            if step in (0, 24, 25, STEPS - 1):
                for k, v in zip(("obs", "rew", "done", "per_agent"), (out[0], out[1], out[2], out[3]._per_agent)):
                    arrays["%s.step%03d.%s" % (name, step, k)] = v
        for k, v in zip(("obs", "rew", "done", "per_agent"), acc):
            arrays["%s.sum.%s" % (name, k)] = v
        for k in env.state_names:
            arrays["%s.state.%s" % (name, k)] = getattr(env, k)
    torch.manual_seed(77)
    for rows, na in ((8192, 5), (4096, 48)):
        logits = torch.randn(rows, na, device="cuda") * 3
        avail = (torch.rand(rows, na, device="cuda") > 0.3).float()
        avail[:, 0] = 1.0
        for tag, av in (("nomask", None), ("mask", avail)):
            a, lp = fused_loss.sample_categorical(logits, av)
            arrays["k14.%dx%d.%s.actions" % (rows, na, tag)], arrays["k14.%dx%d.%s.logp" % (rows, na, tag)] = a, lp
    for heads in ((5, 10), (3, 7, 2)):
        logits = torch.randn(8192, sum(heads), device="cuda") * 3
        a, lp = fused_loss.sample_multi_categorical(logits, heads)
        tag = "x".join(str(h) for h in heads)
        arrays["k14multi.%s.actions" % tag], arrays["k14multi.%s.logp" % tag] = a, lp
    torch.cuda.synchronize()
    for name, t in arrays.items():
        np.save(os.path.join(outdir, name + ".npy"), t.cpu().numpy())
    with open(os.path.join(outdir, "info.json"), "w") as f:
        json.dump({"library": _native.LIB_PATH, "arrays": sorted(arrays)}, f)


def child_time():
    torch, fused_loss, Spread, Reference = _setup()
    gen = torch.Generator().manual_seed(5)
    for env in (Spread(WORLDS, 3, device="cuda", seed=11), Reference(WORLDS, device="cuda", seed=13)):
        env.reset()
        act = _actions(torch, env, gen)
        for _ in range(LAUNCHES):
            env.step(act)
        torch.cuda.synchronize()
    one, two = torch.randn(8192, 5, device="cuda"), torch.randn(8192, 15, device="cuda")
    for _ in range(LAUNCHES):
        fused_loss.sample_categorical(one)
        fused_loss.sample_multi_categorical(two, (5, 10))
    torch.cuda.synchronize()


def _env(lib):
    return dict(os.environ, MAPPO_HIP_LIB=os.path.abspath(lib))


def compare_bits(old, new):
    import numpy as np
    tmp = tempfile.mkdtemp(prefix="ab_mpe_core_")
    record, same_everywhere = {}, True
    try:
        dirs = {}
        for tag, lib in (("old", old), ("new", new)):
            dirs[tag] = os.path.join(tmp, tag)
            os.mkdir(dirs[tag])
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child-bits", dirs[tag]], check=True,
                           env=_env(lib), timeout=600)
            info = json.load(open(os.path.join(dirs[tag], "info.json")))
            assert os.path.samefile(info["library"], lib), info
        assert info["arrays"], "no outputs"
        for name in info["arrays"]:
            a, b = (np.load(os.path.join(dirs[t], name + ".npy")) for t in ("old", "new"))
            same = a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a, b))
            finite = bool(np.isfinite(a).all())
            record[name] = {"shape": list(a.shape), "identical": same, "finite": finite}
            same_everywhere &= same and finite
            if not same:
                print("DIFFERENT", name, record[name], flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print("bits: %d arrays, %s" % (len(record), "all identical" if same_everywhere else "DIFFERENCES"), flush=True)
    return {"identical": bool(same_everywhere), "worlds": WORLDS, "steps": STEPS, "arrays": record}


def kernel_times(lib):
    """-> {kernel: average microseconds per launch} of one --child-time process under rocprofv3."""
    tmp = tempfile.mkdtemp(prefix="ab_mpe_core_prof_")
    try:
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", tmp, "-o", "t", "--", sys.executable,
                        os.path.abspath(__file__), "--child-time"], check=True, env=_env(lib), timeout=300, cwd=tmp,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)[0]
        out = {}
        for row in csv.DictReader(open(stats)):
            for k in KERNELS:       # ("multi_categorical..." is listed before its suffix "categorical...")
                if k in row["Name"]:
                    assert int(row["Calls"]) == LAUNCHES, row
                    out.setdefault(k, round(float(row["AverageNs"]) / 1e3, 3))
                    break
        assert set(out) == set(KERNELS), out
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def bench_ms(lib):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "3"],
                         check=True, env=_env(lib), timeout=600, capture_output=True, text=True).stdout
    return json.loads(out.strip().splitlines()[-1])["ms_per_step"]


def verdict(old, new):
    return {"old": old, "new": new, "old_min": min(old), "old_max": max(old), "new_median": statistics.median(new),
            "within_old_spread": bool(min(old) <= statistics.median(new) <= max(old)),
            "not_slower_than_old_spread": bool(statistics.median(new) <= max(old))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old")
    ap.add_argument("--new", default=os.path.join(ROOT, "on-policy_amd", "lib", "libmappo_hip.so"))
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--bench-pairs", type=int, default=0)
    ap.add_argument("--json")
    ap.add_argument("--child-bits", metavar="DIR")
    ap.add_argument("--child-time", action="store_true")
    opt = ap.parse_args()
    if opt.child_bits:
        return child_bits(opt.child_bits)
    if opt.child_time:
        return child_time()
    assert opt.old, "--old LIBRARY"
    record = {"what": "A / B by library of the particle-world core (one set of physics helpers under spread_step_kernel and "
                      "reference_step_kernel, one sampler body under both K14 kernels): the parent commit's libmappo_hip.so "
                      "(tools/ab_old_lib.sh) against this tree's, each in fresh child processes (tools/ab_mpe_core.py); "
                      "bits = np.array_equal on every output and state tensor, times = rocprofv3 --kernel-trace --stats "
                      "averages over %d launches per process in microseconds, libraries alternating" % LAUNCHES,
              "old": opt.old, "new": opt.new}
    record["bits"] = compare_bits(opt.old, opt.new)
    ok = record["bits"]["identical"]
    series = {k: ([], []) for k in KERNELS}
    for pair in range(opt.pairs):
        for i, lib in enumerate((opt.old, opt.new)):
            for k, us in kernel_times(lib).items():
                series[k][i].append(us)
        print("pair %d:" % pair, {k: (v[0][-1], v[1][-1]) for k, v in series.items()}, flush=True)
    record["kernel_us"] = {k: verdict(*v) for k, v in series.items()} if opt.pairs else {}
    if opt.bench_pairs:
        old_ms, new_ms = [], []
        for pair in range(opt.bench_pairs):
            old_ms.append(bench_ms(opt.old))
            new_ms.append(bench_ms(opt.new))
            print("bench pair %d: old %.3f new %.3f ms per step" % (pair, old_ms[-1], new_ms[-1]), flush=True)
        record["bench_ns_ms_per_step"] = dict(verdict(old_ms, new_ms), command="python bench.py --gpus 1 --steps 10 --warmup 3")
    checks = list(record["kernel_us"].values()) + ([record["bench_ns_ms_per_step"]] if opt.bench_pairs else [])
    record["within_old_spread"] = all(c["within_old_spread"] for c in checks)
    record["not_slower_than_old_spread"] = all(c["not_slower_than_old_spread"] for c in checks)
    ok = ok and record["not_slower_than_old_spread"]
    print(json.dumps({"identical": record["bits"]["identical"], "within_old_spread": record["within_old_spread"],
                      "not_slower_than_old_spread": record["not_slower_than_old_spread"]}))
    if opt.json:
        with open(opt.json, "w") as f:
            json.dump(record, f, indent=1, sort_keys=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
