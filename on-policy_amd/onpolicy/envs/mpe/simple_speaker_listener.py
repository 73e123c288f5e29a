"""Speaker and listener ("simple_speaker_listener") of the multi-agent particle environment, held as tensors on the
policy's device (``TorchParticleWorlds``, particle_worlds.py), like ``TorchSimpleReference`` (simple_reference.py).

Two agents and three coloured landmarks.  Agent 0, the speaker, never moves: it sees the colour of the goal landmark
and says one of three symbols.  Agent 1, the listener, is silent: it sees its own velocity, the landmarks relative to
itself and what the speaker said, and has to reach the goal landmark.  No contact forces.  Semantics follow the
reference's onpolicy/envs/mpe/scenarios/simple_speaker_listener.py (goal, reward, observation), environment.py:115-255
(action decoding, shared reward, done at ``episode_length``) and core.py:160-190 / :207-288 (integration of movable
entities, communication state); trajectories are pinned to the reference's own environment by
tests/test_mpe_speaker_listener_cpu.py (fixtures: tools/make_golden_mpe_speaker_listener.py).

The agents differ in their spaces (the reference's train_mpe_comm.sh runs them with separate policies): the speaker
acts in ``Discrete(3)`` and observes 3 numbers, the listener acts in ``Discrete(5)`` (no-op, +x, -x, +y, -y) and
observes 11.  Observations leave as one row per world, [N, 14] with the speaker's columns first -- the centralised
critic's input as it stands; ``agent_obs(obs, i)`` is agent i's column view.  Reward: ``-|listener - landmark[goal]|^2``
for either agent (``individual_reward``), shared as their sum.
"""
from onpolicy.envs.mpe.particle_worlds import TorchParticleWorlds
from onpolicy.envs.spaces import Discrete

_DIM_C = 3
_MOVES = 5
_SPEAKER, _LISTENER = 0, 1
# landmark colours (scenarios/simple_speaker_listener.py reset_world); the speaker observes the goal landmark's
_PALETTE = ((0.65, 0.15, 0.15), (0.15, 0.65, 0.15), (0.15, 0.15, 0.65))


class TorchSimpleSpeakerListener(TorchParticleWorlds):
    """``n_threads`` simple_speaker_listener worlds as tensors on ``device``.  Besides the particle state: goal [N] (the
    goal landmark's index) and comm [N] (the index of the speaker's last symbol, -1 while silent after a reset).

    Actions: the integer tensor [N, 2] (or [N, 2, 1]) -- column 0 the speaker's symbol, column 1 the listener's
    movement, the two policies' actions side by side -- or the host protocol's one-hots concatenated, [N, 8].  ``step``
    returns obs [N, 14] float32 (see ``obs_dims``), rewards [N, 2, 1] float32, dones [N, 2] bool, infos (lazy).  Kernel
    path: ``mappo_simple_speaker_listener_step`` (K11 family)."""
    state_names = TorchParticleWorlds.state_names + ("goal", "comm")
    obs_dims = (3, 2 + 2 * 3 + _DIM_C)          # columns of an observation row per agent: speaker 0:3, listener 3:14

    def __init__(self, n_threads, num_agents=2, num_landmarks=3, episode_length=25, seed=1, auto_reset=True,
                 device="cpu"):
        assert int(num_agents) == 2, "simple_speaker_listener: only 2 agents are supported"
        assert int(num_landmarks) == 3, "simple_speaker_listener: the landmark palette has 3 colours"
        super().__init__(n_threads, 2, 3, episode_length, seed, auto_reset, device, obs_dim=self.obs_dims,
                         action_space=(Discrete(_DIM_C), Discrete(_MOVES)))
        torch = self._torch
        i64 = dict(dtype=torch.int64, device=self.device)
        self.goal = torch.zeros(self.n, **i64)
        self.comm = torch.full((self.n,), -1, **i64)
        self._palette = torch.tensor(_PALETTE, dtype=torch.float64, device=self.device)
        self._symbols = torch.arange(_DIM_C, **i64)
        self._movable = torch.tensor([False, True], device=self.device).view(1, 2, 1)      # the speaker stays put

    def agent_obs(self, obs, agent_id):
        """Agent ``agent_id``'s own observation: a column view of the rows ``step`` / ``reset`` return."""
        lo = sum(self.obs_dims[:agent_id])
        return obs[..., lo:lo + self.obs_dims[agent_id]]

    def _obs_shape(self):
        return (self.n, sum(self.obs_dims))

    def _fresh(self):
        """Agent positions U(-1, 1), landmarks U(-1, 1), the goal."""
        return super()._fresh() + (self._torch.randint(0, self.l, (self.n,), generator=self.rng, device=self.device),)

    def _restart(self, which, fresh):
        torch = self._torch
        super()._restart(which, fresh)
        self.goal = torch.where(which, fresh[2], self.goal)
        self.comm = torch.where(which, torch.full_like(self.comm, -1), self.comm)

    def _indices(self, actions):
        """-> (the speaker's symbol [N], the listener's movement [N]) int64 from index actions [N, 2] / [N, 2, 1] or
        the concatenated one-hots [N, 8]."""
        if actions.shape == (self.n, _DIM_C + _MOVES):                      # one-hot (the host protocol)
            return actions[:, :_DIM_C].argmax(-1), actions[:, _DIM_C:].argmax(-1)
        assert actions.shape in ((self.n, 2), (self.n, 2, 1)), tuple(actions.shape)
        idx = actions.reshape(self.n, 2).to(self._torch.int64)
        return idx[:, _SPEAKER], idx[:, _LISTENER]

    def _obs(self):
        torch = self._torch
        colour = self._palette[self.goal]                                                    # [N, 3]
        rel_land = (self.landmarks - self.pos[:, _LISTENER, None, :]).reshape(self.n, -1)    # [N, 6]
        heard = (self.comm[:, None] == self._symbols).to(torch.float64)                      # [N, 3]
        return torch.cat([colour, self.vel[:, _LISTENER], rel_land, heard], -1).to(torch.float32)

    def _reward(self):
        goal_pos = self.landmarks.gather(1, self.goal.view(-1, 1, 1).expand(self.n, 1, 2))[:, 0]     # [N, 2]
        d2 = ((self.pos[:, _LISTENER] - goal_pos) ** 2).sum(-1)
        return -d2[:, None].expand(self.n, 2)

    def _forces(self, actions):
        torch = self._torch
        sym, move = self._indices(actions)
        self.comm = sym.clone()             # the symbol becomes the communication state
        push = self._directions[move]       # on the listener alone
        return torch.stack([torch.zeros_like(push), push], 1)

    def _kernel_actions(self, actions):
        if actions.shape == (self.n, _DIM_C + _MOVES):
            return self._torch.stack(self._indices(actions), -1)
        assert actions.shape in ((self.n, 2), (self.n, 2, 1)), tuple(actions.shape)
        return actions.reshape(self.n, 2)

    def _launch(self, idx, fresh, obs, rewards, dones, per_agent):
        from onpolicy import _native
        p = _native.ptr
        fresh_pos, fresh_land, fresh_goal = fresh or (None, None, None)
        _native.check(_native.lib().mappo_simple_speaker_listener_step(
            p(self.pos), p(self.vel), p(self.landmarks), p(self.t), p(self.goal), p(self.comm), p(idx), p(fresh_pos),
            p(fresh_land), p(fresh_goal), p(obs), p(rewards), p(dones), p(per_agent), self.n, self.world_length,
            int(self.auto_reset), _native.stream_of(self.device)), "mappo_simple_speaker_listener_step")
