"""Referential communication ("simple_reference") of the multi-agent particle environment, held as tensors on the
policy's device (``TorchParticleWorlds``, particle_worlds.py), like ``TorchSimpleSpread`` (simple_spread.py).

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
from onpolicy.envs.mpe.particle_worlds import TorchParticleWorlds
from onpolicy.utils.multi_discrete import MultiDiscrete

_DIM_C = 10
_MOVES = 5
# landmark colours (scenarios/simple_reference.py reset_world); an agent observes its goal landmark's
_PALETTE = ((0.75, 0.25, 0.25), (0.25, 0.75, 0.25), (0.25, 0.25, 0.75))


class TorchSimpleReference(TorchParticleWorlds):
    """``n_threads`` simple_reference worlds as tensors on ``device``.  Besides the particle state: goal [N, 2] (the goal
    landmark's index per agent) and comm [N, 2] (the index of the agent's last communication symbol, -1 while silent
    after a reset).

    Actions: the integer tensor [N, 2, 2] (movement, symbol) as it comes out of the policy, or the host protocol's
    concatenated one-hot [N, 2, 15].  ``step`` returns obs [N, 2, 21] float32, rewards [N, 2, 1] float32, dones [N, 2]
    bool, infos (lazy).  Kernel path: ``mappo_simple_reference_step`` (K11 family)."""
    state_names = TorchParticleWorlds.state_names + ("goal", "comm")
    landmark_scale = 0.8

    def __init__(self, n_threads, num_agents=2, num_landmarks=3, episode_length=25, seed=1, auto_reset=True,
                 device="cpu"):
        assert int(num_agents) == 2, "simple_reference: only 2 agents are supported"
        assert int(num_landmarks) == 3, "simple_reference: the landmark palette has 3 colours"
        super().__init__(n_threads, 2, 3, episode_length, seed, auto_reset, device, obs_dim=2 + 2 * 3 + 3 + _DIM_C,
                         action_space=lambda: MultiDiscrete([[0, _MOVES - 1], [0, _DIM_C - 1]]))
        torch = self._torch
        i64 = dict(dtype=torch.int64, device=self.device)
        self.goal = torch.zeros(self.n, self.a, **i64)
        self.comm = torch.full((self.n, self.a), -1, **i64)
        self._palette = torch.tensor(_PALETTE, dtype=torch.float64, device=self.device)
        self._symbols = torch.arange(_DIM_C, **i64)

    def _fresh(self):
        """Agent positions U(-1, 1), landmarks U(-1, 1) (scaled by 0.8 where used), goals."""
        return super()._fresh() + (self._torch.randint(0, self.l, (self.n, self.a), generator=self.rng,
                                                       device=self.device),)

    def _restart(self, which, fresh):
        torch = self._torch
        super()._restart(which, fresh)
        self.goal = torch.where(which.view(-1, 1), fresh[2], self.goal)
        self.comm = torch.where(which.view(-1, 1), torch.full_like(self.comm, -1), self.comm)

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

    def _forces(self, actions):
        move, sym = self._indices(actions)
        self.comm = sym.clone()             # the symbol becomes the communication state; no contacts in this scenario
        return self._directions[move]

    def _kernel_actions(self, actions):
        if actions.shape == (self.n, self.a, _MOVES + _DIM_C):
            return self._torch.stack(self._indices(actions), -1)
        assert actions.shape == (self.n, self.a, 2), tuple(actions.shape)
        return actions

    def _launch(self, idx, fresh, obs, rewards, dones, per_agent):
        from onpolicy import _native
        p = _native.ptr
        fresh_pos, fresh_land, fresh_goal = fresh or (None, None, None)
        _native.check(_native.lib().mappo_simple_reference_step(
            p(self.pos), p(self.vel), p(self.landmarks), p(self.t), p(self.goal), p(self.comm), p(idx), p(fresh_pos),
            p(fresh_land), p(fresh_goal), p(obs), p(rewards), p(dones), p(per_agent), self.n, self.world_length,
            int(self.auto_reset), _native.stream_of(self.device)), "mappo_simple_reference_step")
