"""-m gpu: K11 wide for simple_push (``mappo_simple_push_step_wide``): keep-away worlds of up to 64 agents as one launch,
the lanes of a wave along a world's agents -- against the tensor-op step, and under the captured rollout.  With
MAPPO_MARGINS_JSON=<path> the worst deviation of every case is merged into that file (``k11_push_wide.*`` of
profiles/small_kernel_margins.json)."""
import json
import os

import pytest
import torch

from test_mpe_push_cpu import push_argv

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


@pytest.mark.parametrize("agents,landmarks,worlds", [
    (17, 2, 65),        # the first count past the thin kernel: 32 lanes, odd Dg, odd rows; the last workgroup holds one world
    (2, 1, 193),        # the smallest world: even Dg, a good agent with no other good agent
    (32, 2, 3),         # every lane of a half wave busy
    (33, 1, 5),         # 64 lanes, half idle; the second workgroup partly filled
    (64, 2, 5),         # every lane busy, a row of 9,139 floats: many trips per lane
    (3, 2, 64)])        # the reference script's shape, which the thin kernel takes too
def test_wide_step_equals_tensor_ops(agents, landmarks, worlds):
    """Every step on its own against ``_step_ops`` in float64 from the same seed and the same state (the reference's
    state is copied into the kernel's tensors after each step, or a trajectory would amplify the last bits in which the
    two orders of summation differ).  State and per_agent to 1e-12, the bound test_gpu_mpe_tag_wide derives for 127
    contact terms per agent: here at most 63, of at most 1e2 * 0.1, a few ulp each, times dt 0.1.  The step compares
    nothing with a threshold (soft contacts, a minimum), so no state has to be avoided.  The first worlds start with
    agents 0 and 1 in contact, the last with agents 0 and A - 1 at one point (no force between them, on either path).  The
    kernel must have run: the state tensors stay where they are."""
    from onpolicy.envs.mpe.simple_push import TorchSimplePush
    T = 7
    a, b = (TorchSimplePush(worlds, agents, landmarks, seed=5, device=DEV, world_length=T, wide=wide)
            for wide in (True, False))
    assert a.graph_safe and a._wide and not b._wide
    assert torch.equal(a.reset(), b.reset())
    touching = slice(0, (worlds + 1) // 2)
    for env in (a, b):
        env.pos[touching, 1] = env.pos[touching, 0] + torch.tensor([0.03, 0.04], dtype=torch.float64, device=DEV)
        env.pos[worlds - 1, agents - 1] = env.pos[worlds - 1, 0]
    where = [getattr(a, name).data_ptr() for name in a.state_names]
    worst = MARGINS.setdefault("k11_push_wide.a%d_l%d_n%d" % (agents, landmarks, worlds),
                               {"bound": "atol 1e-12 vs the float64 tensor step", "pos": 0.0, "vel": 0.0,
                                "landmarks": 0.0, "per_agent": 0.0})
    g = torch.Generator(device=DEV).manual_seed(1)
    for step in range(3 * T + 2):
        act = torch.randint(0, 5, (worlds, agents), generator=g, device=DEV)
        if step % 2:        # the host protocol's one-hot actions are accepted too
            act = torch.nn.functional.one_hot(act, 5).float()
        ra, rb = a.step(act), b._step_ops(act)
        got = dict(pos=a.pos, vel=a.vel, landmarks=a.landmarks, per_agent=ra[3]._per_agent)
        want = dict(pos=b.pos, vel=b.vel, landmarks=b.landmarks, per_agent=rb[3]._per_agent)
        for name in got:
            worst[name] = max(worst[name], float((got[name] - want[name]).abs().max()))
        torch.testing.assert_close(ra[0], rb[0], rtol=0, atol=1e-6)
        torch.testing.assert_close(ra[1], rb[1], rtol=0, atol=1e-6)
        assert torch.equal(ra[2], rb[2]) and torch.equal(a.t, b.t) and torch.equal(a.goal, b.goal)
        for name in got:
            torch.testing.assert_close(got[name], want[name], rtol=0, atol=1e-12, msg=lambda m: name + ": " + m)
        for name in a.state_names:
            getattr(a, name).copy_(getattr(b, name))
    assert where == [getattr(a, name).data_ptr() for name in a.state_names]


def _run(tmp_path, monkeypatch, graph):
    from onpolicy.scripts.train import train_mpe
    monkeypatch.setenv("MAPPO_RESULTS_DIR", str(tmp_path / ("results" + graph)))
    monkeypatch.setenv("MAPPO_ROLLOUT_GRAPH", graph)
    monkeypatch.setenv("MAPPO_PUSH_WIDE", "1")
    threads = torch.get_num_threads()
    try:
        return train_mpe.main(push_argv("mappo", 3, n=8, steps=2 * 8 * 25, hidden=64) + ["--use_device_env"])
    finally:
        torch.set_num_threads(threads)      # (--n_training_threads 1 sets the process's thread count)


def test_rollout_through_the_wide_kernel_is_captured(tmp_path, monkeypatch):
    """Under MAPPO_PUSH_WIDE=1 the separated rollout step captures with the wide kernel in it, and the captured run fills
    every agent's buffer as the eager one."""
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
    from onpolicy.envs.mpe.simple_push import TorchSimplePush
    assert TorchSimplePush(3, 17, 2, device=DEV, wide=True).graph_safe
    assert not TorchSimplePush(3, 17, 2, device=DEV).graph_safe
