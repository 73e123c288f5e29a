"""Referential communication ("simple_reference") of the multi-agent particle environment, held as tensors on the
policy's device, like ``TorchSimpleSpread`` (simple_spread.py).

Two agents and three coloured landmarks.  Each agent is assigned a goal landmark that the OTHER agent has to reach:
it sees its goal's colour, not its position, and tells the other agent through a 10-symbol communication channel.
The physics are simple_spread's without contact forces.  Semantics follow the reference's
onpolicy/envs/mpe/scenarios/simple_reference.py (goals, reward, observation), environment.py:115-255 (MultiDiscrete
action decoding, shared reward, done at ``episode_length``) and core.py:207-288 (integration, communication state);
trajectories are pinned to the reference's own environment by tests/test_mpe_reference_cpu.py (fixtures:
tools/make_golden_mpe_reference.py).

Action space ``MultiDiscrete([[0, 4], [0, 9]])``: a movement (no-op, +x, -x, +y, -y) and a communication symbol per
agent.  Observation of agent i (21): own velocity (2), landmarks relative to the agent (6), the colour of its own goal
landmark (3), the other agent's communication state as a one-hot (10).  Reward: ``r_i = -|pos_other -
landmark[goal_i]|^2``, shared (both agents receive r_0 + r_1; ``individual_reward`` is r_i).
"""
from onpolicy.envs.spaces import Box
from onpolicy.envs.mpe.simple_spread import _DAMPING, _DT, _SENSITIVITY, _LazyInfos
from onpolicy.utils.multi_discrete import MultiDiscrete

_DIM_C = 10
_MOVES = 5
_LANDMARK_SCALE = 0.8
# landmark colours (scenarios/simple_reference.py reset_world); an agent observes its goal landmark's
_PALETTE = ((0.75, 0.25, 0.25), (0.25, 0.75, 0.25), (0.25, 0.25, 0.75))


class TorchSimpleReference(object):
    """``n_threads`` simple_reference worlds as tensors on ``device``.  State is float64 like the reference's numpy
    physics: pos / vel [N, 2, 2], landmarks [N, 3, 2], t [N], goal [N, 2] (the goal landmark's index per agent) and
    comm [N, 2] (the index of the agent's last communication symbol, -1 while silent after a reset); observations and
    rewards leave as float32.

    ``device_resident = True``: the runner hands over the integer actions [N, 2, 2] (movement, symbol) as they come out
    of the policy; the host protocol's concatenated one-hot [N, 2, 15] is accepted as well.  ``step`` returns obs
    [N, 2, 21] float32, rewards [N, 2, 1] float32, dones [N, 2] bool, infos (lazy).  On a HIP device a step is one
    launch (``mappo_simple_reference_step``, K11 family) that advances the state in place; ``_step_ops`` is the same
    step as tensor operations (any device) and consumes the same generator draws."""
    device_resident = True
    # the tensors a captured rollout graph snapshots / restores and expects to stay in place (runner/shared/rollout_graph.py)
    state_names = ("pos", "vel", "landmarks", "t", "goal", "comm")

    def __init__(self, n_threads, num_agents=2, num_landmarks=3, episode_length=25, seed=1, auto_reset=True,
                 device="cpu"):
        import torch
        self._torch = torch
        assert int(num_agents) == 2, "simple_reference: only 2 agents are supported"
        assert int(num_landmarks) == 3, "simple_reference: the landmark palette has 3 colours"
        self.auto_reset = auto_reset
        self.device = torch.device(device)
        self.n, self.a, self.l = int(n_threads), 2, 3
        self.world_length = int(episode_length)
        self.rng = torch.Generator(device=self.device)
        self.rng.manual_seed(int(seed))
        self.obs_dim = 2 + 2 * self.l + 3 + _DIM_C
        self.observation_space = [Box(shape=(self.obs_dim,)) for _ in range(self.a)]
        self.share_observation_space = [Box(shape=(self.obs_dim * self.a,)) for _ in range(self.a)]
        self.action_space = [MultiDiscrete([[0, _MOVES - 1], [0, _DIM_C - 1]]) for _ in range(self.a)]
        f64 = dict(dtype=torch.float64, device=self.device)
        i64 = dict(dtype=torch.int64, device=self.device)
        self.pos = torch.zeros(self.n, self.a, 2, **f64)
        self.vel = torch.zeros(self.n, self.a, 2, **f64)
        self.landmarks = torch.zeros(self.n, self.l, 2, **f64)
        self.t = torch.zeros(self.n, **i64)
        self.goal = torch.zeros(self.n, self.a, **i64)
        self.comm = torch.full((self.n, self.a), -1, **i64)
        # action index -> force direction (environment.py: u[0] += a[1] - a[2], u[1] += a[3] - a[4])
        self._directions = torch.tensor([[0, 0], [1, 0], [-1, 0], [0, 1], [0, -1]], **f64) * _SENSITIVITY
        self._palette = torch.tensor(_PALETTE, **f64)
        self._symbols = torch.arange(_DIM_C, **i64)

    # -- random draws: the same calls, in the same order, on both step paths
    def _fresh(self):
        """Reset draws for every world: agent positions U(-1, 1), landmarks U(-1, 1) (scaled by 0.8 where used), goals."""
        torch = self._torch
        pos = torch.empty(self.n, self.a, 2, dtype=torch.float64, device=self.device).uniform_(-1.0, 1.0,
                                                                                                generator=self.rng)
        land = torch.empty(self.n, self.l, 2, dtype=torch.float64, device=self.device).uniform_(-1.0, 1.0,
                                                                                                 generator=self.rng)
        goal = torch.randint(0, self.l, (self.n, self.a), generator=self.rng, device=self.device)
        return pos, land, goal

    def _reset_worlds(self, which):
        """Branch-free (no host sync): fresh state is drawn for every world and kept where ``which`` is set."""
        torch = self._torch
        pos, land, goal = self._fresh()
        w = which.view(-1, 1, 1)
        self.pos = torch.where(w, pos, self.pos)
        self.vel = torch.where(w, torch.zeros_like(self.vel), self.vel)
        self.landmarks = torch.where(w, _LANDMARK_SCALE * land, self.landmarks)
        self.goal = torch.where(which.view(-1, 1), goal, self.goal)
        self.comm = torch.where(which.view(-1, 1), torch.full_like(self.comm, -1), self.comm)
        self.t = torch.where(which, torch.zeros_like(self.t), self.t)

    def _indices(self, actions):
        """-> (movement [N, 2], symbol [N, 2]) int64 from index actions [N, 2, 2] or one-hot [N, 2, 15]."""
        torch = self._torch
        if actions.shape == (self.n, self.a, _MOVES + _DIM_C):            # one-hot (the host protocol)
            return actions[..., :_MOVES].argmax(-1), actions[..., _MOVES:].argmax(-1)
        assert actions.shape == (self.n, self.a, 2), tuple(actions.shape)
        idx = actions.to(torch.int64)
        return idx[..., 0], idx[..., 1]

    def _obs(self):
        torch = self._torch
        rel_land = (self.landmarks[:, None, :, :] - self.pos[:, :, None, :]).reshape(self.n, self.a, -1)
        colour = self._palette[self.goal]                                             # [N, 2, 3]
        heard = (self.comm.flip(1)[..., None] == self._symbols).to(torch.float64)     # the other agent's symbol
        return torch.cat([self.vel, rel_land, colour, heard], -1).to(torch.float32)

    def _reward(self):
        goal_pos = self.landmarks.gather(1, self.goal[..., None].expand(self.n, self.a, 2))    # [N, 2, 2]
        return -((self.pos.flip(1) - goal_pos) ** 2).sum(-1)                                   # [N, 2]

    def reset(self):
        torch = self._torch
        self._reset_worlds(torch.ones(self.n, dtype=torch.bool, device=self.device))
        return self._obs()

    @property
    def graph_safe(self):
        """True when ``step`` advances the state tensors IN PLACE (the kernel path): a captured rollout graph may replay it."""
        return self.device.type == "cuda"

    def step(self, actions):
        actions = self._torch.as_tensor(actions, device=self.device)
        if self.device.type == "cuda":
            return self._step_kernel(actions)
        return self._step_ops(actions)

    def _step_kernel(self, actions):
        """The whole step as one launch (``mappo_simple_reference_step``): the arithmetic and generator draws of
        ``_step_ops``."""
        torch = self._torch
        from onpolicy import _native
        if actions.shape == (self.n, self.a, _MOVES + _DIM_C):
            idx = torch.stack(self._indices(actions), -1)
        else:
            assert actions.shape == (self.n, self.a, 2), tuple(actions.shape)
            idx = actions.to(torch.int64).contiguous()
        fresh_pos, fresh_land, fresh_goal = self._fresh() if self.auto_reset else (None, None, None)
        obs = torch.empty(self.n, self.a, self.obs_dim, dtype=torch.float32, device=self.device)
        rewards = torch.empty(self.n, self.a, 1, dtype=torch.float32, device=self.device)
        dones = torch.empty(self.n, self.a, dtype=torch.bool, device=self.device)
        per_agent = torch.empty(self.n, self.a, dtype=torch.float64, device=self.device)
        for name in self.state_names:
            setattr(self, name, getattr(self, name).contiguous())
        p = _native.ptr
        _native.check(_native.lib().mappo_simple_reference_step(
            p(self.pos), p(self.vel), p(self.landmarks), p(self.t), p(self.goal), p(self.comm), p(idx), p(fresh_pos),
            p(fresh_land), p(fresh_goal), p(obs), p(rewards), p(dones), p(per_agent), self.n, self.world_length,
            int(self.auto_reset), _native.stream_of(self.device)), "mappo_simple_reference_step")
        return obs, rewards, dones, _LazyInfos(per_agent)

    def _step_ops(self, actions):
        torch = self._torch
        move, sym = self._indices(actions)
        u = self._directions[move]
        self.vel = self.vel * (1 - _DAMPING) + u * _DT
        self.pos = self.pos + self.vel * _DT
        self.comm = sym.clone()
        self.t = self.t + 1
        per_agent = self._reward()
        rewards = per_agent.sum(-1, keepdim=True).expand(self.n, self.a).unsqueeze(-1).to(torch.float32)
        done_env = self.t >= self.world_length
        dones = done_env[:, None].expand(self.n, self.a)
        if self.auto_reset:
            self._reset_worlds(done_env)
        return self._obs(), rewards, dones, _LazyInfos(per_agent)

    def close(self):
        pass
