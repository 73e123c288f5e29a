#!/usr/bin/env python
"""What the compiler put BETWEEN the matrix instructions of the six-term K9 kernels: for named kernel instances of
mappo_mlp.hip, the listing's MFMA count, how many of the gaps between two consecutive MFMAs hold nothing but s_nop /
scalar instructions ("empty": the MFMAs issue in a burst and the vector work sits somewhere else, serialised with them),
and an estimate of the issue cycles that no MFMA hides.  From ``hipcc -S --cuda-device-only`` (cross-compiles, no GPU).

Cost model (one wave's stream on one SIMD, the issue costs measured on the MI355X): 4 cycles per vector, LDS or memory
instruction, 8 per transcendental, 1 per scalar instruction (s_nop n: n + 1); a v_mfma_f32_32x32x16_bf16 occupies the
pipe for 32 cycles and hides at most 24 cycles of other issue of the same wave, past which every instruction adds its
full cost.  exposed = sum over the gaps of max(0, cost - 24).  It is an estimate of the LISTING, in listing order: every
gap counts once whatever the trip count of the loop it sits in, and the instructions before the first and after the
last MFMA do not count.  Good for comparing two schedules of the same code, not a time.

    python tools/mfma_gaps.py                  # print the table
    python tools/mfma_gaps.py --write          # refresh "now" in profiles/mfma_gaps.json (keeps its "parent" figures)
    python tools/mfma_gaps.py --write --as-parent     # run on the parent commit's tree: refresh "parent" instead
    python tools/mfma_gaps.py --asm mlp.s --gaps 'mlp_fwd4_kernel<1, 4, true>'        # every gap of one instance
"""
import argparse
import json
import os
import re
import subprocess
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "on-policy_amd", "csrc")
SNAPSHOT = os.path.join(ROOT, "profiles", "mfma_gaps.json")
SOURCE = "mappo_mlp.hip"
# the two launches that read the critic's 384-wide rows, then the other six-term instances of the same templates
CRITIC = ("mlp_fwd4_kernel<1, 4, true>", "mlp_dw1_direct_kernel<3, 2, true>")
KERNELS = CRITIC + ("mlp_fwd4_kernel<0, 4, true>", "mlp_fwd4_kernel<2, 4, true>", "mlp_fwd4_kernel<1, 1, true>",
                    "mlp_dw1_direct_kernel<4, 2, true>", "mlp_dw1_direct_kernel<3, 4, true>")
HIDDEN = 24                 # issue cycles of the same wave that one 32-cycle MFMA hides
TRANSCENDENTAL = ("v_exp_", "v_log_", "v_rcp_", "v_rsq_", "v_sqrt_", "v_sin_", "v_cos_")
PACKED_F32 = re.compile(r"^v_pk_(add|mul|fma)_f32$")


def assembly():
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
           "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only", os.path.join(CSRC, SOURCE), "-o", "-"]
    return subprocess.run(cmd, capture_output=True, text=True, check=True).stdout


def kernel_bodies(text):
    """{demangled kernel name without its argument list: [instruction lines]} of every kernel in the listing"""
    mangled = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)
    plain = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True,
                           check=True).stdout.splitlines()
    names = {}
    for m, p in zip(mangled, plain):
        p = re.sub(r"^void\s+", "", p)
        p = re.sub(r"\((?:[^()]|\([^()]*\))*\)$", "", p)            # the argument list
        names[m] = re.sub(r"^(?:\w+::|\(anonymous namespace\)::)+", "", p)
    bodies, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^(\w+):", line)
        if m and m.group(1) in names:
            cur = bodies.setdefault(names[m.group(1)], [])
            continue
        if cur is None:
            continue
        s = line.strip()
        if s.startswith(".Lfunc_end") or s.startswith(".section") or s.startswith(".amdhsa_kernel"):
            cur = None
            continue
        if not line.startswith("\t") or not s or s[0] in ".;":
            continue
        cur.append(s)
    return bodies


def cost(op, operands):
    if op == "s_nop":
        return int(operands.split()[0]) + 1 if operands.split() else 1
    if op.startswith("s_"):
        return 1
    if op.startswith(TRANSCENDENTAL):
        return 8
    return 4


def gaps_of(body):
    """[(instructions, vector-side instructions, cost)] of every stretch between two consecutive MFMAs"""
    gaps, n, nvec, c, started = [], 0, 0, 0, False
    for ins in body:
        op, _, rest = ins.partition(" ")
        if op.startswith("v_mfma_"):
            if started:
                gaps.append((n, nvec, c))
            started, n, nvec, c = True, 0, 0, 0
        else:
            n += 1
            nvec += not op.startswith("s_")
            c += cost(op, rest)
    return gaps


def measure(body):
    ops = Counter(ins.split(" ", 1)[0] for ins in body)
    gaps = gaps_of(body)
    return {
        "mfma": sum(v for k, v in ops.items() if k.startswith("v_mfma_")),
        "mfma_bf16": sum(v for k, v in ops.items() if k.startswith("v_mfma_") and k.endswith("_bf16")),
        "gaps": len(gaps),
        "gaps_empty": sum(1 for g in gaps if g[1] == 0),
        "gaps_over_hidden": sum(1 for g in gaps if g[2] > HIDDEN),
        "largest_gap_cycles": max([g[2] for g in gaps] or [0]),
        "exposed_cycles": sum(max(0, g[2] - HIDDEN) for g in gaps),
        "s_nop": ops.get("s_nop", 0),
        "packed_f32": sum(v for k, v in ops.items() if PACKED_F32.match(k)),
    }


def collect(text=None):
    bodies = kernel_bodies(assembly() if text is None else text)
    missing = [k for k in KERNELS if k not in bodies]
    assert not missing, "not in the listing: %s" % missing
    return {k: measure(bodies[k]) for k in KERNELS}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--as-parent", action="store_true", help="with --write: store the figures under 'parent'")
    ap.add_argument("--asm", help="read this listing instead of compiling")
    ap.add_argument("--gaps", metavar="KERNEL", help="print every gap of one instance and stop")
    opt = ap.parse_args()
    text = open(opt.asm).read() if opt.asm else assembly()
    if opt.gaps:
        body = kernel_bodies(text)[opt.gaps]
        for i, (n, nvec, c) in enumerate(gaps_of(body)):
            print("gap %4d: %4d instructions (%4d vector), %5d cycles" % (i, n, nvec, c))
        raise SystemExit(0)
    table = collect(text)
    for k, row in table.items():
        print(k, row)
    if opt.write:
        snap = json.load(open(SNAPSHOT)) if os.path.exists(SNAPSHOT) else {}
        snap["model"] = {"hidden_cycles_per_mfma": HIDDEN, "vector_lds_memory": 4, "transcendental": 8, "scalar": 1}
        snap["parent" if opt.as_parent else "now"] = table
        with open(SNAPSHOT, "w") as f:
            json.dump(snap, f, indent=1, sort_keys=True)
        print("wrote", SNAPSHOT)
