"""-m gpu: ``train_mpe.py --use_device_eval``.  The evaluation step replayed from its captured graph against the eager
tensor loop (twin runners: logged values, totals, every eval-world state tensor, bit for bit), an evaluation that leaves
training untouched, and the framework's deterministic action (``MAPPO_FUSED_SAMPLE=0``) behind the same loop."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
N, T = 5, 6                         # worlds (training and eval), episode length; hidden 64 so that K9 runs
SCENARIOS = ("simple_spread", "simple_reference", "simple_speaker_listener")


def _argv(scenario, algo, episodes, extra=()):
    agents = "3" if scenario == "simple_spread" else "2"
    argv = ["--env_name", "MPE", "--scenario_name", scenario, "--num_agents", agents, "--num_landmarks", "3",
            "--algorithm_name", algo, "--seed", "1", "--n_rollout_threads", str(N), "--episode_length", str(T),
            "--num_env_steps", str(episodes * N * T), "--ppo_epoch", "2", "--num_mini_batch", "1",
            "--data_chunk_length", "3", "--hidden_size", "64", "--gain", "0.01", "--lr", "7e-4", "--critic_lr", "7e-4",
            "--use_wandb", "--log_interval", "1", "--n_training_threads", "1", "--use_device_env"]
    if scenario == "simple_speaker_listener":
        argv.append("--share_policy")           # store_false: one policy per agent
    return argv + list(extra)


EVAL = ("--use_eval", "--use_device_eval", "--eval_interval", "1", "--n_eval_rollout_threads", str(N))


def _runner(tmp_path, monkeypatch, name, scenario, algo, episodes=1, extra=EVAL, graph="1"):
    from onpolicy.scripts.train import train_mpe
    monkeypatch.setenv("MAPPO_RESULTS_DIR", str(tmp_path / name))
    monkeypatch.setenv("MAPPO_EVAL_GRAPH", graph)
    return train_mpe.main(_argv(scenario, algo, episodes, extra))


def _policies(runner):
    return runner.policy if isinstance(runner.policy, list) else [runner.policy]


def _logged(runner, step):
    rows = [json.loads(l) for l in open(os.path.join(runner.log_dir, "scalars.jsonl"))]
    return sorted((r["tag"], r[r["tag"]]) for r in rows if r["step"] == step and "eval_average_episode_rewards" in r["tag"])


def _align(src, dst):
    """``dst`` evaluates what ``src`` evaluates: the same actors, the same eval worlds and generator, in place."""
    for ps, pd in zip(_policies(src), _policies(dst)):
        pd.actor.load_state_dict(ps.actor.state_dict())
    for name in src.eval_envs.state_names:
        getattr(dst.eval_envs, name).copy_(getattr(src.eval_envs, name))
    dst.eval_envs.rng.set_state(src.eval_envs.rng.get_state())


@pytest.mark.parametrize("algo", ["rmappo", "mappo"])
@pytest.mark.parametrize("scenario", SCENARIOS)
def test_captured_eval_equals_eager_eval(tmp_path, monkeypatch, scenario, algo):
    """Two evaluations in a row -- after a train(), so with updated weights; the second (every one after the first) resets
    the worlds under a live graph -- replayed from the captured step and run by the eager tensor loop."""
    g = _runner(tmp_path, monkeypatch, "graph", scenario, algo, graph="1")
    e = _runner(tmp_path, monkeypatch, "eager", scenario, algo, graph="0")
    worlds = g.eval_envs
    assert type(worlds).__name__.startswith("Torch") and worlds.device.type == "cuda" and worlds is not g.envs
    assert g.eval_graph is not None and g.eval_graph.graph is not None, "the eval step was not captured"
    assert e.eval_graph is None
    assert g.eval_graph.replays == T                      # the evaluation inside main(): captured there, replayed since
    _align(g, e)
    ptrs = {name: getattr(worlds, name).data_ptr() for name in worlds.state_names}
    for call in (0, 1):
        g.eval(5000 + call)
        e.eval(5000 + call)
        torch.cuda.synchronize()
        got, want = _logged(g, 5000 + call), _logged(e, 5000 + call)
        assert len(want) == (2 if scenario == "simple_speaker_listener" else 1) and got == want, (got, want)
        assert g.eval_totals.shape == e.eval_totals.shape and torch.equal(g.eval_totals, e.eval_totals)
        assert float(g.eval_totals.max()) < 0.0
        for name in worlds.state_names:
            assert torch.equal(getattr(worlds, name), getattr(e.eval_envs, name)), (call, name)
        assert torch.equal(worlds.rng.get_state(), e.eval_envs.rng.get_state())
    assert g.eval_graph.replays == T + 2 * T              # 2 x episode_length replays for the two calls
    assert ptrs == {name: getattr(worlds, name).data_ptr() for name in worlds.state_names}
    # the auto-reset at the end of an episode left fresh worlds; the totals differ between the calls (other worlds)
    assert int(worlds.t.sum()) == 0


def test_evaluation_does_not_perturb_training(tmp_path, monkeypatch):
    """Two episodes of simple_spread with an evaluation after each, and without any: the same weights, bit for bit."""
    a = _runner(tmp_path, monkeypatch, "with", "simple_spread", "rmappo", episodes=2)
    b = _runner(tmp_path, monkeypatch, "without", "simple_spread", "rmappo", episodes=2, extra=())
    assert a.eval_graph is not None and a.eval_graph.replays == 2 * T and b.eval_envs is None
    for net in ("actor", "critic"):
        sa, sb = getattr(a.policy, net).state_dict(), getattr(b.policy, net).state_dict()
        assert sorted(sa) == sorted(sb)
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (net, k)
    for name in a.envs.state_names:
        assert torch.equal(getattr(a.envs, name), getattr(b.envs, name)), name
    assert torch.equal(a.envs.rng.get_state(), b.envs.rng.get_state())


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_eval_without_the_mode_kernel_logs_the_same(tmp_path, monkeypatch, scenario):
    """``MAPPO_FUSED_SAMPLE=0`` takes the mode kernel away: the device eval runs on the framework's ops and logs the
    same value (equal actions => equal rewards; a seed that meets a tie is replaced, not tolerated)."""
    from onpolicy import _native
    r = _runner(tmp_path, monkeypatch, "fallback", scenario, "rmappo", graph="0")
    assert r.eval_graph is None
    state = {name: getattr(r.eval_envs, name).clone() for name in r.eval_envs.state_names}
    rng = r.eval_envs.rng.get_state()
    logged = {}
    for mode in ("1", "0"):
        for name, kept in state.items():
            getattr(r.eval_envs, name).copy_(kept)
        r.eval_envs.rng.set_state(rng)
        monkeypatch.setenv("MAPPO_FUSED_SAMPLE", mode)
        _native.count_calls(True)
        try:
            r.eval(7000 + int(mode))
            calls = _native.calls()
        finally:
            _native.count_calls(False)
        used = calls.get("mappo_categorical_mode", 0) + calls.get("mappo_multi_categorical_mode", 0)
        assert (used > 0) == (mode == "1"), calls
        logged[mode] = ([v for _, v in _logged(r, 7000 + int(mode))], r.eval_totals.clone())
    assert logged["1"][0] and logged["1"][0] == logged["0"][0]
    assert torch.equal(logged["1"][1], logged["0"][1])
