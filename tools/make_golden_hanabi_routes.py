#!/usr/bin/env python
"""TEST INFRASTRUCTURE.  Generates tests/golden/hanabi_route_cases.npz: what the host-tables route of ``HanabiRunner`` plays
with the stub policy of tests/hanabi_turns_common.py (lowest legal move) on the host stepper -- Hanabi-Small, N = 7, T = 8,
``SEEDS``, A = 2 and A = 3, on the CPU.

MUST be run at commit 184a686 ("Hanabi device turns: host-free moves (K17) ..."), the last one at which the runner's
``collect`` held its own text of the bookkeeping after a move.  Since then every route settles a move through
``hanabi_turns.settle_move`` / ``settle_finished``, so the routes' agreement with each other no longer compares independent
texts; this recording is the anchor that shares no code with them.  Regenerating it at a later commit would record the
code under test.

    python tools/make_golden_hanabi_routes.py --out <this tree>/tests/golden      (from a built checkout of 184a686)

Per case ``a<A>_``: the 13 buffer fields after T buffer steps, ``use_rows`` (the current rows, concatenated), and the
counters ``moves`` / ``games`` / ``mean_score``.
"""
import argparse
import os
import pathlib
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "on-policy_amd"), ROOT):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    opt = ap.parse_args()
    os.environ.setdefault("MAPPO_RESULTS_DIR", tempfile.mkdtemp())
    import hanabi_turns_common as common
    import onpolicy.runner.shared.base_runner as base
    from host_buffer import HostSharedBuffer
    from onpolicy.envs.hanabi import batch as hb
    base.SharedReplayBuffer = HostSharedBuffer
    out = {}
    for players in (2, 3):
        args = common.hanabi_args(players)
        envs = hb.HanabiBatchVecEnv(args, common.SEEDS, copy=False)
        runner = common.make_runner(args, envs, torch.device("cpu"), pathlib.Path(tempfile.mkdtemp()) / "run")
        fields, counters = common.play(runner)
        envs.close()
        assert sorted(fields) == sorted(common.BUFFER_FIELDS + ("use_rows",))
        for k, v in fields.items():
            out["a%d_%s" % (players, k)] = v
        out["a%d_moves" % players] = np.int64(counters["moves"])
        out["a%d_games" % players] = np.int64(counters["games"])
        out["a%d_mean_score" % players] = np.float64(counters["mean_score"])
        print("A = %d: %s" % (players, counters))
    path = os.path.join(opt.out, "hanabi_route_cases.npz")
    np.savez_compressed(path, **out)
    print("hanabi_route_cases.npz: %d arrays, %d B" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
