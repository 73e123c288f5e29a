"""Predator-prey ("simple_tag") of the multi-agent particle environment, held as tensors on the policy's device
(``TorchParticleWorlds``, particle_worlds.py), like ``TorchSimplePush`` (simple_push.py).

``num_adversaries`` adversaries, agents 0..Nadv-1, chase the ``G = A - Nadv`` good agents that follow them in agent
order, among ``L`` landmarks that collide and never move.  Every agent moves, is silent and collides.  An adversary is
large and slow (radius 0.075, acceleration 3, top speed 1.0), a good agent small and fast (0.05, 4, 1.3), a landmark has
radius 0.2; every mass is 1.  Semantics follow the reference's onpolicy/envs/mpe/scenarios/simple_tag.py (constants,
rewards, observations), environment.py:115-255 (action decoding, rewards that are NOT shared, done) and core.py:207-321
(action force, integration with the top speed, contact forces between agents and between agents and landmarks);
trajectories are pinned to the reference's own environment by tests/test_mpe_tag_cpu.py (fixtures:
tools/make_golden_mpe_tag.py).

The action force is ``accel ** 2`` times the direction, 9 for an adversary and 16 for a good agent: the reference applies
``accel`` as the action's sensitivity (environment.py:233-236) and again as the force's factor (core.py:236-237).

The agents differ in their observations, so they run with one policy each (the separated runner).  Every agent acts in
``Discrete(5)`` (no-op, +x, -x, +y, -y) and observes its velocity, its position, the landmarks and the other agents
relative to itself and the velocities of the other good agents: 4 + 2 L + 2 (A - 1) + 2 G numbers for an adversary, two
fewer for a good agent.  Observations leave as one row per world, the agents' columns in agent order -- the centralised
critics' input as it stands; ``agent_obs(obs, i)`` is agent i's column view.  Rewards are individual.  With ``hits`` the
number of (good agent, adversary) pairs closer than 0.125 after the step, every adversary is paid ``10 hits``; a good
agent ``-10`` per adversary touching it, minus ``bound(|x|) + bound(|y|)`` for leaving the screen.

The scenario never sets ``world.world_length``, so the reference ends an episode after 25 steps (core.py:137) whatever
``--episode_length`` says; so do these worlds.
"""
from onpolicy.envs.mpe.particle_worlds import TorchParticleWorlds
from onpolicy.envs.spaces import Discrete

_MOVES = 5
_WORLD_LENGTH = 25                      # core.py:137; simple_tag.py leaves it alone
_LANDMARK_SIZE = 0.2
# (adversary, good agent)
_SIZE = (0.075, 0.05)
_ACCEL = (3.0, 4.0)
_MAX_SPEED = (1.0, 1.3)
_CATCH = 10.0
KERNEL_MAX_AGENTS = 16                  # MAPPO_ENV_MAX_ENTITIES
KERNEL_MAX_LANDMARKS = 4                # MAPPO_TAG_MAX_LANDMARKS


def obs_widths(num_adversaries, num_good, num_landmarks):
    """Observation width of every agent, in agent order."""
    a = num_adversaries + num_good
    adversary = 4 + 2 * num_landmarks + 2 * (a - 1) + 2 * num_good
    return (adversary,) * num_adversaries + (adversary - 2,) * num_good


class TorchSimpleTag(TorchParticleWorlds):
    """``n_threads`` simple_tag worlds as tensors on ``device``; no state besides the particle state.

    Actions: the integer tensor [N, A] (or [N, A, 1]), the policies' actions side by side, or the host protocol's
    one-hots, [N, A, 5] or concatenated [N, 5 A].  ``step`` returns obs [N, sum(obs_dims)] float32, rewards [N, A, 1]
    float32 (each agent's own), dones [N, A] bool, infos (lazy).  ``episode_length`` is accepted for the common call
    shape and unused: worlds report done at ``world_length`` steps (None: the reference's 25).  Kernel path:
    ``mappo_simple_tag_step`` (K11 family), up to 16 agents and 4 landmarks; more take the tensor-op path."""
    landmark_scale = 0.8
    shared_reward = False

    def __init__(self, n_threads, num_agents=4, num_landmarks=2, episode_length=25, seed=1, auto_reset=True,
                 device="cpu", world_length=None, num_adversaries=3):
        a, l, adv = int(num_agents), int(num_landmarks), int(num_adversaries)
        assert 1 <= adv < a, "simple_tag: at least one adversary and one good agent (%d adversaries of %d agents)" % (adv, a)
        assert l >= 1, "simple_tag: at least one landmark"
        self.num_adversaries, self.num_good = adv, a - adv
        kind = [0] * adv + [1] * (a - adv)
        super().__init__(n_threads, a, l, _WORLD_LENGTH if world_length is None else world_length, seed, auto_reset,
                         device, obs_dim=obs_widths(adv, a - adv, l), action_space=lambda: Discrete(_MOVES),
                         action_scale=[_ACCEL[k] * _ACCEL[k] for k in kind])
        torch = self._torch
        f64 = dict(dtype=torch.float64, device=self.device)
        size = torch.tensor([_SIZE[k] for k in kind], **f64)
        self._others = ~torch.eye(a, dtype=torch.bool, device=self.device)
        self._dist_min = size[:, None] + size[None, :]                                     # [A, A]
        self._landmark_dist_min = size[:, None] + _LANDMARK_SIZE                           # [A, 1]
        self._max_speed = torch.tensor([_MAX_SPEED[k] for k in kind], **f64).view(1, a, 1)
        self._good_others = self._others[adv:, adv:]                                       # [G, G]

    def agent_obs(self, obs, agent_id):
        """Agent ``agent_id``'s own observation: a column view of the rows ``step`` / ``reset`` return."""
        lo = sum(self.obs_dims[:agent_id])
        return obs[..., lo:lo + self.obs_dims[agent_id]]

    def _obs_shape(self):
        return (self.n, sum(self.obs_dims))

    @property
    def graph_safe(self):
        return self.device.type == "cuda" and self.a <= KERNEL_MAX_AGENTS and self.l <= KERNEL_MAX_LANDMARKS

    def _obs(self):
        torch = self._torch
        n, a, l, adv = self.n, self.a, self.l, self.num_adversaries
        rel_land = (self.landmarks[:, None, :, :] - self.pos[:, :, None, :]).reshape(n, a, 2 * l)
        rel_other = self.pos[:, None, :, :] - self.pos[:, :, None, :]                      # [n, i, j] = pos_j - pos_i
        rel_other = rel_other[:, self._others].reshape(n, a, 2 * (a - 1))
        good_vel = self.vel[:, None, adv:, :].expand(n, a, a - adv, 2)                     # [n, i, g] = vel_g
        common = torch.cat([self.vel, self.pos, rel_land, rel_other], -1)
        adversaries = torch.cat([common[:, :adv], good_vel[:, :adv].reshape(n, adv, -1)], -1)
        others_vel = good_vel[:, adv:][:, self._good_others].reshape(n, a - adv, 2 * (a - adv - 1))
        good = torch.cat([common[:, adv:], others_vel], -1)
        return torch.cat([adversaries.reshape(n, -1), good.reshape(n, -1)], -1).to(torch.float32)

    def _reward(self):
        torch = self._torch
        adv = self.num_adversaries
        delta = self.pos[:, adv:, None, :] - self.pos[:, None, :adv, :]                    # [N, G, Nadv, 2]
        caught = torch.sqrt((delta ** 2).sum(-1)) < self._dist_min[adv:, :adv]
        hits = caught.sum((1, 2)).to(torch.float64)                                        # every pair, for every adversary
        # the screen's edge (simple_tag.py:100-108): 0 below 0.9, a ramp to 1 at 1.0, then exp(2 x - 2) up to 10
        x = self.pos[:, adv:].abs()
        bound = torch.where(x < 0.9, torch.zeros_like(x),
                            torch.where(x < 1.0, (x - 0.9) * 10, torch.exp(2 * x - 2).clamp(max=10.0)))
        good = -_CATCH * caught.sum(2).to(torch.float64) - bound.sum(-1)
        return torch.cat([(_CATCH * hits)[:, None].expand(self.n, adv), good], -1)

    def _indices(self, actions):
        """-> movement indices [N, A] from index actions [N, A] / [N, A, 1] or one-hots [N, A, 5] / [N, 5 A]."""
        if actions.shape in ((self.n, self.a, _MOVES), (self.n, self.a * _MOVES)):         # one-hot (the host protocol)
            return actions.reshape(self.n, self.a, _MOVES).argmax(-1)
        assert actions.shape in ((self.n, self.a), (self.n, self.a, 1)), tuple(actions.shape)
        return actions.reshape(self.n, self.a).to(self._torch.int64)

    def _forces(self, actions):
        return (self._action_forces(self._indices(actions)) + self._contact_forces(self._dist_min)
                + self._landmark_contact_forces(self._landmark_dist_min))

    def _kernel_actions(self, actions):
        return self._indices(actions)

    def _launch(self, idx, fresh, obs, rewards, dones, per_agent):
        from onpolicy import _native
        p = _native.ptr
        fresh_pos, fresh_land = fresh or (None, None)
        _native.check(_native.lib().mappo_simple_tag_step(
            p(self.pos), p(self.vel), p(self.landmarks), p(self.t), p(idx), p(fresh_pos), p(fresh_land), p(obs),
            p(rewards), p(dones), p(per_agent), self.n, self.a, self.num_adversaries, self.l, self.world_length,
            int(self.auto_reset), _native.stream_of(self.device)), "mappo_simple_tag_step")
