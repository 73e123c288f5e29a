"""The device-resident simple_adversary (onpolicy/envs/mpe/simple_adversary.py, tensor-op path on CPU tensors) against
trajectories of the reference's own particle environment (fixtures from tools/make_golden_mpe_adversary.py: free play, a
good agent driven onto the goal, the adversary resting on it); spaces and column views; resets; the registration in the
train script; what the new entry point refuses before anything is launched."""
import ctypes

import numpy as np
import pytest
import torch

from onpolicy import _native
from onpolicy.envs.mpe.simple_adversary import TorchSimpleAdversary, obs_widths

T = 25
CASES = "mpe_adversary_cases"
N_CASES = 6         # 0-3 free play at A = 3, 3, 2, 5; 4 a good agent onto the goal; 5 the adversary on the goal


def _close(got, want, tol, msg):
    np.testing.assert_allclose(got.cpu().numpy() if torch.is_tensor(got) else got, want, rtol=tol, atol=tol, err_msg=msg)


@pytest.mark.parametrize("case", range(N_CASES))
def test_step_ops_matches_reference_trajectories(gold, case):
    """World 0 follows the reference case, world 1 takes random actions (worlds must not interact).  Tolerances: the
    siblings' -- state 1e-9, observations 2e-6, rewards 1e-6."""
    z, key, n = gold.npz(CASES), "adv%d_" % case, 2
    A, L = (int(v) for v in z[key + "dims"])
    env = TorchSimpleAdversary(n, A, num_landmarks=7, episode_length=40, seed=0, auto_reset=False)
    dims = obs_widths(A)
    assert L == A - 1 == env.l and env.world_length == T
    assert env.obs_dims == tuple(z[key + "obs_dims"]) == dims
    assert [s.shape for s in env.share_observation_space] == [tuple(z[key + "share_obs_dim"])] * A == [(sum(dims),)] * A
    assert [(type(s).__name__, s.n) for s in env.action_space] == [("Discrete", d) for d in z[key + "action_dims"]]
    env.reset()
    for name, src in (("pos", "pos0"), ("vel", "vel0"), ("landmarks", "landmarks")):
        getattr(env, name)[0] = torch.from_numpy(np.asarray(z[key + src], dtype=np.float64))
    env.goal[0], env.t[0] = int(z[key + "goal"]), 0
    obs = env._obs()
    for i in range(A):
        _close(env.agent_obs(obs, i)[0], z[key + "obs0_%d" % i], 2e-6, "obs0 agent %d" % i)
    rng = np.random.default_rng(99)
    for t in range(T):
        idx = np.concatenate([z[key + "action_idx"][t][None], rng.integers(0, 5, (n - 1, A))]).astype(np.int64)
        obs, rew, done, info = env._step_ops(torch.from_numpy(idx))
        assert obs.dtype == torch.float32 and obs.shape == (n, sum(dims)) and rew.shape == (n, A, 1)
        msg = "case %d t=%d" % (case, t)
        _close(env.pos[0], z[key + "pos"][t], 1e-9, msg)
        _close(env.vel[0], z[key + "vel"][t], 1e-9, msg)
        for i in range(A):
            _close(env.agent_obs(obs, i)[0], z[key + "obs_%d" % i][t], 2e-6, msg + " agent %d" % i)
        _close(rew[0], z[key + "rewards"][t].reshape(A, 1), 1e-6, msg)
        assert info._per_agent.dtype == torch.float64
        _close(info._per_agent[0], z[key + "individual_rewards"][t], 1e-6, msg)
        np.testing.assert_array_equal(done[0].numpy(), z[key + "dones"][t])
        assert bool(done[0].all()) == (t == T - 1) and int(env.goal[0]) == int(z[key + "goal"])


@pytest.mark.parametrize("a,l,dims", [(2, None, (4, 6)), (3, None, (8, 10, 10)), (5, None, (16,) + (18,) * 4),
                                      (3, 5, (14, 16, 16))])
def test_spaces_widths_and_column_views(a, l, dims):
    env = TorchSimpleAdversary(3, a, landmarks=l, seed=2)
    L = a - 1 if l is None else l
    assert env.obs_dims == dims == obs_widths(a, l) and env._obs_shape() == (3, sum(dims))
    assert [s.shape for s in env.observation_space] == [(d,) for d in dims]
    assert (env.state_names, env.landmark_scale, env.shared_reward) == (("pos", "vel", "landmarks", "t", "goal"), 1.0, False)
    obs = env.reset()
    rows = torch.arange(3)
    adv = env.agent_obs(obs, 0)
    assert adv.shape == (3, dims[0]) and adv._base is obs
    assert torch.equal(adv[:, :2 * L].double().reshape(3, L, 2), (env.landmarks - env.pos[:, :1]).float().double())
    for i in range(1, a):
        o = env.agent_obs(obs, i)
        assert o.shape == (3, dims[i]) and o.data_ptr() == obs[:, sum(dims[:i]):].data_ptr()
        # the goal relative to the agent (0:2) is one of the landmarks relative to it (2:2 + 2 L)
        assert torch.equal(o[:, :2], o[:, 2:2 + 2 * L].reshape(3, L, 2)[rows, env.goal])
        assert torch.equal(o[:, 2 + 2 * L:4 + 2 * L], -adv[:, 2 * L + 2 * (i - 1):2 * L + 2 * i])       # agent 0, mirrored


def test_reset_in_place_equals_reset_at_fixed_addresses():
    a, b = TorchSimpleAdversary(6, 4, seed=8), TorchSimpleAdversary(6, 4, seed=8)
    a.reset(), b.reset()
    for _ in range(3):
        act = torch.randint(0, 5, (6, 4))
        a.step(act), b.step(act)
    kept = {k: getattr(b, k) for k in b.state_names}
    assert torch.equal(a.reset(), b.reset_in_place())
    for k in a.state_names:
        assert torch.equal(getattr(a, k), getattr(b, k)) and getattr(b, k) is kept[k], k
    assert torch.equal(a.rng.get_state(), b.rng.get_state())
    assert float(a.landmarks.abs().max()) > 0.8                     # uniform(-1, 1), no 0.8 scale (24 draws)


def test_registration_and_device_env_refusals(monkeypatch, tmp_path):
    from onpolicy.scripts.train import _launch, train_mpe
    assert train_mpe.DEVICE_ENVS["simple_adversary"] is TorchSimpleAdversary
    assert "simple_adversary" in train_mpe.SEPARATED_DEVICE_ENVS and "simple_adversary" not in train_mpe.KIND_DEFAULTS
    monkeypatch.setattr(_launch, "device_of", lambda all_args: torch.device("cpu"))
    monkeypatch.setenv("MAPPO_RESULTS_DIR", str(tmp_path / "results"))
    argv = ["--env_name", "MPE", "--experiment_name", "check", "--scenario_name", "simple_adversary", "--num_agents", "3",
            "--n_rollout_threads", "2", "--use_wandb", "--use_device_env"]
    for extra in (["--algorithm_name", "mappo"],                            # the shared-policy runner
                  ["--algorithm_name", "happo", "--share_policy"]):
        with pytest.raises(NotImplementedError, match="use_device_env"):
            train_mpe.main(argv + extra)
    with pytest.raises(NotImplementedError, match="needs a HIP device"):    # the separated runner, but a CPU device
        train_mpe.main(argv + ["--algorithm_name", "mappo", "--share_policy"])
    for bad in (dict(num_agents=1), dict(landmarks=0), dict(num_agents=65), dict(landmarks=65)):
        with pytest.raises(AssertionError, match="simple_adversary"):
            TorchSimpleAdversary(4, **bad)


@pytest.mark.parametrize("agents,landmarks,null,code", [(1, 1, None, -2), (3, 0, None, -2), (65, 2, None, -4),
                                                        (3, 65, None, -4), (3, 2, 0, -1), (3, 2, 4, -1), (3, 2, 8, -1)])
def test_entry_refuses_bad_calls(agents, landmarks, null, code):
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)       # validation returns before anything is enqueued: a host buffer serves as pointer
    ptrs = [None if i == null else p for i in range(13)]        # 0 pos, 4 goal, 8 fresh_goal (with auto_reset)
    assert _native.lib().mappo_simple_adversary_step(*ptrs, 4, agents, landmarks, 25, 1, None) == code
    assert not any(buf)
