"""Physical deception ("simple_adversary") of the multi-agent particle environment, held as tensors on the policy's
device (``TorchParticleWorlds``, particle_worlds.py), like ``TorchSimplePush`` (simple_push.py).

``A`` agents and ``L`` landmarks, one of which is the goal all agents share.  Agent 0, the adversary, is paid for being
close to the goal but is not told which landmark it is; the good agents 1..A-1 know it and are paid for covering it while
the adversary stays away.  Every agent moves and is silent and nothing collides, so the force on an agent is its action's
alone.  Semantics follow the reference's onpolicy/envs/mpe/scenarios/simple_adversary.py (goal, rewards, observations),
environment.py:115-255 (action decoding, rewards that are NOT shared, done) and core.py:160-190 / :207-288
(integration); trajectories are pinned to the reference's own environment by tests/test_mpe_adversary_cpu.py (fixtures:
tools/make_golden_mpe_adversary.py).

The agents differ in their observations, so they run with one policy each (the separated runner).  Every agent acts in
``Discrete(5)`` (no-op, +x, -x, +y, -y).  Observations hold positions only: the adversary sees the landmarks and the other
agents relative to itself, 2 L + 2 (A - 1) numbers; a good agent the goal relative to itself and then the same two blocks,
2 + 2 L + 2 (A - 1) numbers.  They leave as one row per world, the adversary's columns first and then the good agents' in
agent order -- the centralised critics' input as it stands; ``agent_obs(obs, i)`` is agent i's column view.  Rewards are
individual: with d_i = |pos_i - goal|, ``-d_0 ** 2`` for the adversary and ``d_0 - min over good agents d_g`` for every
good agent.

The reference's scenario builds A - 1 landmarks whatever ``--num_landmarks`` says, at uniform(-1, 1) (simple_push's 0.8
scale is not used here), and never sets ``world.world_length``, so an episode is 25 steps (core.py:137) whatever
``--episode_length`` says; so do these worlds.
"""
from onpolicy.envs.mpe.particle_worlds import TorchParticleWorlds
from onpolicy.envs.spaces import Discrete

_MOVES = 5
_ADVERSARY = 0
_WORLD_LENGTH = 25          # core.py:137; simple_adversary.py leaves it alone
_MAX_ENTITIES = 64          # MAPPO_ENV_WIDE_MAX_ENTITIES: a world's agents, and its landmarks, lie along one wave


def obs_widths(num_agents, landmarks=None):
    """-> each agent's observation width: (Da,) + (Dg,) * (A - 1)."""
    a = int(num_agents)
    l = a - 1 if landmarks is None else int(landmarks)
    return (2 * l + 2 * (a - 1),) + (2 + 2 * l + 2 * (a - 1),) * (a - 1)


class TorchSimpleAdversary(TorchParticleWorlds):
    """``n_threads`` simple_adversary worlds as tensors on ``device``.  Besides the particle state: goal [N] (the goal
    landmark's index).

    Actions: the integer tensor [N, A] (or [N, A, 1]), the policies' actions side by side, or the host protocol's
    one-hots, [N, A, 5] or concatenated [N, 5 A].  ``step`` returns obs [N, sum(obs_dims)] float32, rewards [N, A, 1]
    float32 (each agent's own), dones [N, A] bool, infos (lazy).  ``num_landmarks`` and ``episode_length`` are accepted
    for the common call shape and unused, as the reference ignores them: a world has ``landmarks`` landmarks (None: the
    reference's A - 1) and reports done at ``world_length`` steps (None: the reference's 25).  Kernel path:
    ``mappo_simple_adversary_step`` (K11 family), one kernel for 2 to 64 agents and 1 to 64 landmarks; there is no
    tensor-op route past that on a HIP device, so larger worlds are refused here."""
    state_names = TorchParticleWorlds.state_names + ("goal",)
    landmark_scale = 1.0
    shared_reward = False

    def __init__(self, n_threads, num_agents=3, num_landmarks=None, episode_length=25, seed=1, auto_reset=True,
                 device="cpu", world_length=None, landmarks=None):
        a = int(num_agents)
        l = a - 1 if landmarks is None else int(landmarks)
        assert a >= 2, "simple_adversary: one adversary and at least one good agent"
        assert l >= 1, "simple_adversary: at least one landmark, the goal"
        assert a <= _MAX_ENTITIES and l <= _MAX_ENTITIES, (
            "simple_adversary: at most %d agents and %d landmarks" % (_MAX_ENTITIES, _MAX_ENTITIES))
        super().__init__(n_threads, a, l, _WORLD_LENGTH if world_length is None else world_length, seed, auto_reset,
                         device, obs_dim=obs_widths(a, l), action_space=lambda: Discrete(_MOVES))
        torch = self._torch
        self.goal = torch.zeros(self.n, dtype=torch.int64, device=self.device)
        self._others = ~torch.eye(a, dtype=torch.bool, device=self.device)

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
        super()._restart(which, fresh)
        self.goal = self._torch.where(which, fresh[2], self.goal)

    def _goal_pos(self):
        return self.landmarks.gather(1, self.goal.view(-1, 1, 1).expand(self.n, 1, 2))                # [N, 1, 2]

    def _obs(self):
        torch = self._torch
        n, a, l = self.n, self.a, self.l
        rel_land = (self.landmarks[:, None, :, :] - self.pos[:, :, None, :]).reshape(n, a, 2 * l)
        rel_other = self.pos[:, None, :, :] - self.pos[:, :, None, :]                      # [n, i, j] = pos_j - pos_i
        rel_other = rel_other[:, self._others].reshape(n, a, 2 * (a - 1))
        good = slice(1, a)
        rel_goal = self._goal_pos() - self.pos[:, good]                                    # [N, A - 1, 2]
        adversary = torch.cat([rel_land[:, _ADVERSARY], rel_other[:, _ADVERSARY]], -1)
        others = torch.cat([rel_goal, rel_land[:, good], rel_other[:, good]], -1)
        return torch.cat([adversary, others.reshape(n, -1)], -1).to(torch.float32)

    def _reward(self):
        torch = self._torch
        delta = self.pos - self._goal_pos()
        d2 = delta[..., 0] ** 2 + delta[..., 1] ** 2                                       # [N, A]
        d = torch.sqrt(d2)
        good = d[:, _ADVERSARY] - d[:, 1:].min(-1).values
        return torch.cat([-d2[:, :1], good[:, None].expand(self.n, self.a - 1)], -1)

    def _indices(self, actions):
        """-> movement indices [N, A] from index actions [N, A] / [N, A, 1] or one-hots [N, A, 5] / [N, 5 A]."""
        if actions.shape in ((self.n, self.a, _MOVES), (self.n, self.a * _MOVES)):         # one-hot (the host protocol)
            return actions.reshape(self.n, self.a, _MOVES).argmax(-1)
        assert actions.shape in ((self.n, self.a), (self.n, self.a, 1)), tuple(actions.shape)
        return actions.reshape(self.n, self.a).to(self._torch.int64)

    def _forces(self, actions):
        return self._directions[self._indices(actions)]

    def _kernel_actions(self, actions):
        return self._indices(actions)

    def _launch(self, idx, fresh, obs, rewards, dones, per_agent):
        from onpolicy import _native
        p = _native.ptr
        fresh_pos, fresh_land, fresh_goal = fresh or (None, None, None)
        _native.check(_native.lib().mappo_simple_adversary_step(
            p(self.pos), p(self.vel), p(self.landmarks), p(self.t), p(self.goal), p(idx), p(fresh_pos), p(fresh_land),
            p(fresh_goal), p(obs), p(rewards), p(dones), p(per_agent), self.n, self.a, self.l, self.world_length,
            int(self.auto_reset), _native.stream_of(self.device)), "mappo_simple_adversary_step")
