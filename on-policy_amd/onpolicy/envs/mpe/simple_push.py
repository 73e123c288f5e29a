"""Keep-away ("simple_push") of the multi-agent particle environment, held as tensors on the policy's device
(``TorchParticleWorlds``, particle_worlds.py), like ``TorchSimpleSpeakerListener`` (simple_speaker_listener.py).

``A`` agents and ``L`` coloured landmarks, one of which is the goal all agents share.  Agent 0, the adversary, has to
keep the good agents 1..A-1 away from the goal without being told which landmark it is; the good agents know it.  Every
agent moves, is silent and collides (radius 0.05: soft contact forces below distance 0.1).  Semantics follow the
reference's onpolicy/envs/mpe/scenarios/simple_push.py (goal, rewards, observations), environment.py:115-255 (action
decoding, rewards that are NOT shared, done) and core.py:160-190 / :290-321 (integration, contact forces);
trajectories are pinned to the reference's own environment by tests/test_mpe_push_cpu.py (fixtures:
tools/make_golden_mpe_push.py).

The agents differ in their observations, so they run with one policy each (the separated runner).  Every agent acts in
``Discrete(5)`` (no-op, +x, -x, +y, -y).  The adversary observes its velocity, the landmarks and the other agents
relative to itself, 2 + 2 L + 2 (A - 1) numbers; a good agent its velocity, the goal relative to itself, its own colour
(which names the goal), the landmarks relative to itself, their colours and the other agents relative to itself,
7 + 5 L + 2 (A - 1) numbers.  Observations leave as one row per world, the adversary's columns first and then the good
agents' in agent order -- the centralised critics' input as it stands; ``agent_obs(obs, i)`` is agent i's column view.
Rewards are individual: ``-|pos - goal|`` for a good agent, ``min over good agents |pos_g - goal| - |pos - goal|`` for
the adversary.

The scenario never sets ``world.world_length``, so the reference ends an episode after 25 steps (core.py:137) whatever
``--episode_length`` says; so do these worlds.
"""
from onpolicy.envs.mpe.particle_worlds import TorchParticleWorlds
from onpolicy.envs.spaces import Discrete

_MOVES = 5
_ADVERSARY = 0
_AGENT_SIZE = 0.05
_WORLD_LENGTH = 25          # core.py:137; simple_push.py leaves it alone
_MAX_LANDMARKS = 2          # landmark l is coloured on channel l + 1 of three (simple_push.py:43-45)


class TorchSimplePush(TorchParticleWorlds):
    """``n_threads`` simple_push worlds as tensors on ``device``.  Besides the particle state: goal [N] (the goal
    landmark's index).

    Actions: the integer tensor [N, A] (or [N, A, 1]), the policies' actions side by side, or the host protocol's
    one-hots, [N, A, 5] or concatenated [N, 5 A].  ``step`` returns obs [N, sum(obs_dims)] float32, rewards [N, A, 1]
    float32 (each agent's own), dones [N, A] bool, infos (lazy).  ``episode_length`` is accepted for the common call
    shape and unused: worlds report done at ``world_length`` steps (None: the reference's 25).  Kernel path:
    ``mappo_simple_push_step`` (K11 family), up to 16 agents; more take the tensor-op path."""
    state_names = TorchParticleWorlds.state_names + ("goal",)
    landmark_scale = 0.8
    shared_reward = False

    def __init__(self, n_threads, num_agents=2, num_landmarks=2, episode_length=25, seed=1, auto_reset=True,
                 device="cpu", world_length=None):
        a, l = int(num_agents), int(num_landmarks)
        assert a >= 2, "simple_push: one adversary and at least one good agent"
        assert 1 <= l <= _MAX_LANDMARKS, "simple_push: the landmark palette has %d colours" % _MAX_LANDMARKS
        dims = (2 + 2 * l + 2 * (a - 1),) + (7 + 5 * l + 2 * (a - 1),) * (a - 1)
        super().__init__(n_threads, a, l, _WORLD_LENGTH if world_length is None else world_length, seed, auto_reset,
                         device, obs_dim=dims, action_space=lambda: Discrete(_MOVES))
        torch = self._torch
        f64 = dict(dtype=torch.float64, device=self.device)
        self.goal = torch.zeros(self.n, dtype=torch.int64, device=self.device)
        self._others = ~torch.eye(a, dtype=torch.bool, device=self.device)
        # landmark l: 0.1 with + 0.8 on channel l + 1; a good agent: 0.25 with + 0.5 on channel goal + 1
        channel = torch.eye(3, **f64)[1:1 + l]                                             # [L, 3]
        self._landmark_colours = (0.1 + 0.8 * channel).reshape(1, 1, 3 * l)
        self._agent_colours = 0.25 + 0.5 * channel

    def agent_obs(self, obs, agent_id):
        """Agent ``agent_id``'s own observation: a column view of the rows ``step`` / ``reset`` return."""
        lo = sum(self.obs_dims[:agent_id])
        return obs[..., lo:lo + self.obs_dims[agent_id]]

    def _obs_shape(self):
        return (self.n, sum(self.obs_dims))

    @property
    def graph_safe(self):
        return self.device.type == "cuda" and self.a <= 16

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
        colour = self._agent_colours[self.goal][:, None, :].expand(n, a - 1, 3)
        adversary = torch.cat([self.vel[:, _ADVERSARY], rel_land[:, _ADVERSARY], rel_other[:, _ADVERSARY]], -1)
        others = torch.cat([self.vel[:, good], rel_goal, colour, rel_land[:, good],
                            self._landmark_colours.expand(n, a - 1, 3 * l), rel_other[:, good]], -1)
        return torch.cat([adversary, others.reshape(n, -1)], -1).to(torch.float32)

    def _reward(self):
        torch = self._torch
        d = torch.sqrt(((self.pos - self._goal_pos()) ** 2).sum(-1))                       # [N, A] distance to the goal
        adversary = d[:, 1:].min(-1).values - d[:, _ADVERSARY]
        return torch.cat([adversary[:, None], -d[:, 1:]], -1)

    def _indices(self, actions):
        """-> movement indices [N, A] from index actions [N, A] / [N, A, 1] or one-hots [N, A, 5] / [N, 5 A]."""
        if actions.shape in ((self.n, self.a, _MOVES), (self.n, self.a * _MOVES)):         # one-hot (the host protocol)
            return actions.reshape(self.n, self.a, _MOVES).argmax(-1)
        assert actions.shape in ((self.n, self.a), (self.n, self.a, 1)), tuple(actions.shape)
        return actions.reshape(self.n, self.a).to(self._torch.int64)

    def _forces(self, actions):
        return self._directions[self._indices(actions)] + self._contact_forces(2 * _AGENT_SIZE)

    def _kernel_actions(self, actions):
        return self._indices(actions)

    def _launch(self, idx, fresh, obs, rewards, dones, per_agent):
        from onpolicy import _native
        p = _native.ptr
        fresh_pos, fresh_land, fresh_goal = fresh or (None, None, None)
        _native.check(_native.lib().mappo_simple_push_step(
            p(self.pos), p(self.vel), p(self.landmarks), p(self.t), p(self.goal), p(idx), p(fresh_pos), p(fresh_land),
            p(fresh_goal), p(obs), p(rewards), p(dones), p(per_agent), self.n, self.a, self.l, self.world_length,
            int(self.auto_reset), _native.stream_of(self.device)), "mappo_simple_push_step")
