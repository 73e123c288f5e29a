#!/usr/bin/env python
"""Are two builds of libmappo_hip.so the SAME function on the K9 trunk?  Runs mappo_mlp_forward and mappo_mlp_backward
(six-term arithmetic, the default) at the critic's shape (din 384 / out 1) and the actor's (din 48 / out 5) on seeded
inputs, rows gathered through a permuted row table, once per library in two fresh child processes, and compares every
output bit for bit (np.array_equal): the values, the saved activations of both layers (normalised activations and
{mean, rstd}), and every parameter gradient.  A re-scheduling of the kernels keeps all of them; anything else does not.

    python tools/ab_k9_bits.py --old on-policy_amd/lib/libmappo_hip_OLD.so [--new on-policy_amd/lib/libmappo_hip.so]
                               [--rows 1048576] [--json OUT.json]
Exit status 0: identical everywhere; 1: a difference (printed per array).
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ((384, 1), (48, 5))


def child(din, out, rows, outdir):
    sys.path.insert(0, os.path.join(ROOT, "on-policy_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    from onpolicy import _native
    from onpolicy.algorithms.utils import fused_mlp
    from onpolicy.algorithms.utils.mlp import MLPBase
    from helpers import make_args
    dev = torch.device("cuda", 0)
    torch.manual_seed(1234 + din)
    base = MLPBase(make_args(hidden_size=64, layer_N=1, use_ReLU=False), (din,)).to(dev)
    head = torch.nn.Linear(64, out).to(dev)
    src_rows = rows + 4096
    src = torch.randn(src_rows, din, device=dev)
    xhat = fused_mlp.standardize_rows(src)
    idx = torch.randperm(src_rows, device=dev)[:rows]
    rs = fused_mlp.RowSource(xhat, idx, standardized=True)
    dy = torch.randn(rows, out, device=dev)
    y = fused_mlp.trunk_forward(base, rs, head)
    saved = y.grad_fn.saved_tensors
    params = list(base.parameters()) + list(head.parameters())
    y.backward(dy)
    torch.cuda.synchronize()
    arrays = {"y": y.detach(), "z": saved[0][:, :rows], "ln_stats": saved[1][:, :rows]}
    for i, p in enumerate(params):
        if p.grad is not None:
            arrays["grad_%02d_%s" % (i, "x".join(str(s) for s in p.shape))] = p.grad
    for name, t in arrays.items():
        np.save(os.path.join(outdir, name + ".npy"), t.cpu().numpy())
    with open(os.path.join(outdir, "info.json"), "w") as f:
        json.dump({"library": _native.LIB_PATH, "build": _native.lib().mappo_build_info().decode(),
                   "arrays": sorted(arrays)}, f)


def run_child(lib, din, out, rows, outdir):
    env = dict(os.environ, MAPPO_HIP_LIB=os.path.abspath(lib))
    subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(din), str(out), str(rows), outdir],
                   check=True, env=env, timeout=600)
    return json.load(open(os.path.join(outdir, "info.json")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old")
    ap.add_argument("--new", default=os.path.join(ROOT, "on-policy_amd", "lib", "libmappo_hip.so"))
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--json")
    ap.add_argument("--child", nargs=4, metavar=("DIN", "OUT", "ROWS", "DIR"))
    opt = ap.parse_args()
    if opt.child:
        din, out, rows = (int(v) for v in opt.child[:3])
        return child(din, out, rows, opt.child[3])
    import numpy as np
    assert opt.old, "--old LIBRARY"
    record = {"rows": opt.rows, "old": opt.old, "new": opt.new, "cases": []}
    same_everywhere = True
    for din, out in CASES:
        tmp = tempfile.mkdtemp(prefix="ab_k9_bits_")
        try:
            dirs = {}
            for tag, lib in (("old", opt.old), ("new", opt.new)):
                dirs[tag] = os.path.join(tmp, tag)
                os.mkdir(dirs[tag])
                info = run_child(lib, din, out, opt.rows, dirs[tag])
                assert os.path.samefile(info["library"], lib), info
            case = {"din": din, "out": out, "arrays": {}}
            assert info["arrays"], "no outputs"
            for name in info["arrays"]:
                a = np.load(os.path.join(dirs["old"], name + ".npy"), mmap_mode="r")
                b = np.load(os.path.join(dirs["new"], name + ".npy"), mmap_mode="r")
                same = a.shape == b.shape and bool(np.array_equal(a, b))
                finite = bool(np.isfinite(a).all())
                row = {"shape": list(a.shape), "identical": same, "finite": finite}
                if not same and a.shape == b.shape:
                    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
                    row["differing"] = int((np.asarray(a) != np.asarray(b)).sum())
                    row["max_abs_diff"] = float(d.max())
                case["arrays"][name] = row
                same_everywhere &= same and finite
                print("din %d out %d %-22s %-18s %s" % (din, out, name, tuple(a.shape),
                                                        "identical" if same else "DIFFERENT %s" % row), flush=True)
            record["cases"].append(case)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    record["identical"] = bool(same_everywhere)
    print(json.dumps({"identical": record["identical"], "rows": opt.rows}))
    if opt.json:
        with open(opt.json, "w") as f:
            json.dump(record, f, indent=1, sort_keys=True)
    return 0 if same_everywhere else 1


if __name__ == "__main__":
    sys.exit(main())
