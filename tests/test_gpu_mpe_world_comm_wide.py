"""-m gpu: K11 wide for simple_world_comm (``mappo_simple_world_comm_step_wide``): worlds of up to 64 agents and 60
obstacles as one launch, the lanes of a wave along a world's entities -- against the tensor-op step, and under the
captured rollout.  With MAPPO_MARGINS_JSON=<path> the worst deviation of every case is merged into that file
(``k11_world_comm_wide.*`` of profiles/small_kernel_margins.json)."""
import json
import os

import numpy as np
import pytest
import torch

from test_gpu_mpe_world_comm import _near, _thresholds
from test_mpe_world_comm_cpu import CATCH, FOOD, make, one_hot_actions, random_actions, world_comm_argv

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
MARGINS = {}


@pytest.fixture(autouse=True, scope="module")
def _record_margins():
    yield
    path = os.environ.get("MAPPO_MARGINS_JSON")
    if path and MARGINS:
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc.update(MARGINS)
        with open(path, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)


@pytest.mark.parametrize("adv,good,obstacles,worlds", [
    (13, 4, 2, 65),         # the first agent count past the thin kernel; 32 lanes per world, the last wave half filled
    (4, 2, 5, 3),           # the first obstacle count past it
    (24, 8, 28, 3),         # 32 lanes per world, all busy as agents and as landmarks
    (30, 3, 2, 1),          # 64 lanes per world by the agents alone, a single world
    (2, 3, 36, 65),         # 64 lanes per world by the landmarks, more good agents than adversaries
    (48, 16, 60, 5),        # every lane busy, the second workgroup partly filled, a row of many trips
    (1, 1, 1, 193),         # the smallest world: an empty block of other good agents' velocities
    (4, 2, 1, 64)])         # the reference script's shape, which the thin kernel takes too
def test_wide_step_equals_tensor_ops(adv, good, obstacles, worlds):
    """Every step on its own against ``_step_ops`` in float64 from the same seed and the same state (the reference's
    state is copied into the kernel's tensors after each step, or a trajectory would amplify the last bits in which the
    two orders of summation differ).  State and per_agent to 1e-12, the bound of the simple_tag wide test: at most 123
    contact terms per agent of at most 1e2 * 0.275, a few ulp each, times dt 0.1.  The step's discontinuities are a
    catch (0.12), a meal (0.075) and hiding (0.375 / 0.345): no such distance of the reference, where the rewards or the
    observations read it, may sit within 1e-9 of its threshold.  Three restarts; one-hot actions on odd steps.  The
    kernel must have run: the state tensors stay where they are."""
    agents, T = adv + good, 7
    a, b = (make(worlds, adv, good, obstacles, seed=5, device=DEV, world_length=T, wide=wide) for wide in (True, False))
    assert a.graph_safe and a._wide and not b._wide
    assert torch.equal(a.reset(), b.reset())
    where = [getattr(a, name).data_ptr() for name in a.state_names]
    seen, reward = dict(near=0, caught=0, fed=0, hidden=0), b._reward
    def watched():      # (the state the rewards see: after the physics, before a restart)
        pair, food, _, _ = _thresholds(b)
        seen.update(near=seen["near"] + _near(b), caught=seen["caught"] + int((pair < CATCH).sum()),
                    fed=seen["fed"] + int((food < FOOD).sum()))
        return reward()
    b._reward = watched
    worst = MARGINS.setdefault("k11_world_comm_wide.%dv%d_l%d_n%d" % (adv, good, obstacles, worlds),
                               {"bound": "atol 1e-12 vs the float64 tensor step", "pos": 0.0, "vel": 0.0,
                                "landmarks": 0.0, "per_agent": 0.0})
    g = np.random.default_rng(1)
    for step in range(3 * T + 2):
        act = torch.from_numpy(random_actions(g, worlds, agents)).to(DEV)
        if step % 2:        # the host protocol's one-hot actions are accepted too
            act = one_hot_actions(act).float()
        ra, rb = a.step(act), b._step_ops(act)
        seen["near"] += _near(b)                    # (the state the observations see)
        seen["hidden"] += int((~b.visible()).sum())
        assert seen["near"] == 0, "a distance within 1e-9 of 0.12, 0.075, 0.375 or 0.345: choose another seed"
        got = dict(pos=a.pos, vel=a.vel, landmarks=a.landmarks, per_agent=ra[3]._per_agent)
        want = dict(pos=b.pos, vel=b.vel, landmarks=b.landmarks, per_agent=rb[3]._per_agent)
        for name in got:
            worst[name] = max(worst[name], float((got[name] - want[name]).abs().max()))
        torch.testing.assert_close(ra[0], rb[0], rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(ra[1], rb[1], rtol=1e-6, atol=1e-6)
        assert torch.equal(ra[2], rb[2]) and torch.equal(a.t, b.t) and torch.equal(a.comm, b.comm)
        for name in got:
            torch.testing.assert_close(got[name], want[name], rtol=0, atol=1e-12, msg=lambda m: name + ": " + m)
        for name in a.state_names:
            getattr(a, name).copy_(getattr(b, name))
    assert seen["caught"] > 0 and seen["hidden"] > 0 and (worlds < 64 or seen["fed"] > 0), seen
    assert where == [getattr(a, name).data_ptr() for name in a.state_names]


def _run(tmp_path, monkeypatch, graph):
    from onpolicy.scripts.train import train_mpe
    monkeypatch.setenv("MAPPO_RESULTS_DIR", str(tmp_path / ("results" + graph)))
    monkeypatch.setenv("MAPPO_ROLLOUT_GRAPH", graph)
    monkeypatch.setenv("MAPPO_WORLD_COMM_WIDE", "1")
    threads = torch.get_num_threads()
    try:
        return train_mpe.main(world_comm_argv("mappo", 2, 1, n=8, steps=2 * 8 * 25, hidden=64) + ["--use_device_env"])
    finally:
        torch.set_num_threads(threads)      # (--n_training_threads 1 sets the process's thread count)


def test_rollout_through_the_wide_kernel_is_captured(tmp_path, monkeypatch):
    """Under MAPPO_WORLD_COMM_WIDE=1 the separated rollout step captures with the wide kernel in it, and the captured
    run fills every agent's buffer as the eager one."""
    captured, eager = _run(tmp_path, monkeypatch, "1"), _run(tmp_path, monkeypatch, "0")
    rg = captured.rollout_graph
    assert captured.envs._wide and eager.envs._wide and len(captured.buffer) == 3
    assert rg is not None and rg.graph is not None, "the rollout step was not captured"
    assert rg.replays == 2 * 25
    for got, want in zip(captured.buffer, eager.buffer):
        for name in ("actions", "rewards", "masks", "obs"):
            assert torch.equal(getattr(got, name), getattr(want, name)), name
        for name in ("value_preds", "action_log_probs"):
            torch.testing.assert_close(getattr(got, name), getattr(want, name), rtol=1e-5, atol=1e-6)


def test_wide_is_opt_in():
    assert make(3, 13, 4, 2, device=DEV, wide=True).graph_safe
    assert not make(3, 13, 4, 2, device=DEV).graph_safe
