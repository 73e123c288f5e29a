"""Predator-prey with forests, food and a speaking leader ("simple_world_comm") of the multi-agent particle environment,
held as tensors on the policy's device (``TorchParticleWorlds``, particle_worlds.py), like ``TorchSimpleTag``
(simple_tag.py).

``num_adversaries`` adversaries, agents 0..Nadv-1, chase the ``G = A - Nadv`` good agents that follow them in agent
order.  Agent 0 is the adversaries' leader: it sees everybody and says one of 4 words per step, which every adversary
hears.  An adversary is large and slow (radius 0.075, acceleration 3, top speed 1.0), a good agent small and fast (0.045,
4, 1.3); every mass is 1, every agent collides.  The landmarks are one list: ``L = num_landmarks`` obstacles (radius 0.2,
the only ones that collide), then 2 pieces of food (0.03), then 2 forests (0.3); all restart at 0.8 U(-1, 1).  Semantics
follow the reference's onpolicy/envs/mpe/scenarios/simple_world_comm.py (constants, rewards, observations),
environment.py:54-98 and :115-255 (spaces, action decoding, rewards that are NOT shared, done) and core.py:207-321 (action
force, communication state, integration with the top speed, contact forces); trajectories are pinned to the reference's
own environment by tests/test_mpe_world_comm_cpu.py (fixtures: tools/make_golden_mpe_world_comm.py).

The action force is ``accel ** 2`` times the direction, as in simple_tag.  The leader acts in
``MultiDiscrete([[0, 4], [0, 3]])``, a movement and a word; every other agent in ``Discrete(5)``.  After a step ``comm``
is the leader's word, after a reset nothing has been said (-1: the observation's four columns are zero).

Agent i is ``inside`` forest f when it is closer to the forest's centre than the sum of their radii.  Agent i sees agent
j iff i is the leader, or both are inside forest 0, or both are inside forest 1, or neither is inside any forest: an agent
in a forest does not see one in the open.  An agent that is not seen contributes (0, 0) for its relative position and,
where it is good, for its velocity.

Observation of an adversary: own velocity, own position, the L + 4 landmarks and the other agents relative to itself
(masked), the good agents' velocities (masked), whether it is inside forest 0 / forest 1 as +-1, the leader's word as a
one-hot: 4 + 2 (L + 4) + 2 (A - 1) + 2 G + 6 numbers.  Of a good agent: velocity, position, landmarks, other agents
(masked), the two forest flags, the other good agents' velocities (masked): 4 + 2 (L + 4) + 2 (A - 1) + 2 + 2 (G - 1).
Observations leave as one row per world, the agents' columns in agent order; ``agent_obs(obs, i)`` is agent i's column
view.  Rewards are individual.  With ``hits`` the number of (good agent, adversary) pairs closer than 0.12 after the step,
adversary a is paid ``5 hits - 0.1 min_g |pos_g - pos_a|``; a good agent ``-5`` per adversary touching it, minus twice
``bound(|x|) + bound(|y|)`` for leaving the screen, ``+2`` per food closer than 0.075 and -- positive, as in the
reference -- ``+0.05`` times its distance to the nearest food.

The scenario never sets ``world.world_length``, so the reference ends an episode after 25 steps (core.py:137) whatever
``--episode_length`` says; so do these worlds.
"""
from onpolicy.envs.mpe.particle_worlds import TorchParticleWorlds
from onpolicy.envs.spaces import Discrete
from onpolicy.utils.multi_discrete import MultiDiscrete

_MOVES = 5
_WORDS = 4                              # world.dim_c
_WORLD_LENGTH = 25                      # core.py:137; simple_world_comm.py leaves it alone
_FOOD, _FORESTS = 2, 2
_FIXED = _FOOD + _FORESTS               # the landmarks after the obstacles
_OBSTACLE_SIZE, _FOOD_SIZE, _FOREST_SIZE = 0.2, 0.03, 0.3
# (adversary, good agent)
_SIZE = (0.075, 0.045)
_ACCEL = (3.0, 4.0)
_MAX_SPEED = (1.0, 1.3)
_CATCH = 5.0
_FOOD_REWARD = 2.0
KERNEL_MAX_AGENTS = 16                  # MAPPO_ENV_MAX_ENTITIES
KERNEL_MAX_LANDMARKS = 4                # MAPPO_WORLD_COMM_MAX_OBSTACLES: obstacles; food and forests come on top


def obs_widths(num_adversaries, num_good, num_landmarks):
    """Observation width of every agent, in agent order; ``num_landmarks`` counts the obstacles."""
    a = num_adversaries + num_good
    common = 4 + 2 * (num_landmarks + _FIXED) + 2 * (a - 1) + 2
    return (common + 2 * num_good + _WORDS,) * num_adversaries + (common + 2 * (num_good - 1),) * num_good


class TorchSimpleWorldComm(TorchParticleWorlds):
    """``n_threads`` simple_world_comm worlds as tensors on ``device``.  ``num_landmarks`` counts the obstacles; ``l`` and
    ``landmarks`` cover all ``num_landmarks + 4`` (obstacles, food, forests).  Besides the particle state: comm [N], the
    leader's last word (-1 while nothing has been said since a reset).

    Actions: the integer tensor [N, A + 1], the policies' actions side by side -- the leader's movement, its word, the
    other agents' movements -- or the host protocol's one-hots concatenated, [N, 9 + 5 (A - 1)].  ``step`` returns obs
    [N, sum(obs_dims)] float32, rewards [N, A, 1] float32 (each agent's own), dones [N, A] bool, infos (lazy).
    ``episode_length`` is accepted for the common call shape and unused: worlds report done at ``world_length`` steps
    (None: the reference's 25).  Kernel path: ``mappo_simple_world_comm_step`` (K11 family), up to 16 agents and 4
    obstacles; more take the tensor-op path."""
    state_names = TorchParticleWorlds.state_names + ("comm",)
    landmark_scale = 0.8
    shared_reward = False

    def __init__(self, n_threads, num_agents=6, num_landmarks=1, episode_length=25, seed=1, auto_reset=True,
                 device="cpu", world_length=None, num_adversaries=4):
        a, obstacles, adv = int(num_agents), int(num_landmarks), int(num_adversaries)
        assert 1 <= adv < a, ("simple_world_comm: at least one adversary and one good agent (%d adversaries of %d agents)"
                              % (adv, a))
        assert obstacles >= 1, "simple_world_comm: at least one landmark"
        self.num_adversaries, self.num_good, self.num_obstacles = adv, a - adv, obstacles
        kind = [0] * adv + [1] * (a - adv)
        spaces = [MultiDiscrete([[0, _MOVES - 1], [0, _WORDS - 1]])] + [Discrete(_MOVES) for _ in range(a - 1)]
        super().__init__(n_threads, a, obstacles + _FIXED, _WORLD_LENGTH if world_length is None else world_length, seed,
                         auto_reset, device, obs_dim=obs_widths(adv, a - adv, obstacles), action_space=spaces,
                         action_scale=[_ACCEL[k] * _ACCEL[k] for k in kind])
        torch = self._torch
        f64 = dict(dtype=torch.float64, device=self.device)
        size = torch.tensor([_SIZE[k] for k in kind], **f64)
        self.comm = torch.full((self.n,), -1, dtype=torch.int64, device=self.device)
        self._others = ~torch.eye(a, dtype=torch.bool, device=self.device)
        self._dist_min = size[:, None] + size[None, :]                                     # [A, A]
        # [A, L + 4]: food and forests do not collide (no distance is below -inf: their contact force is an exact zero)
        self._landmark_dist_min = torch.cat([(size[:, None] + _OBSTACLE_SIZE).expand(a, obstacles),
                                             torch.full((a, _FIXED), float("-inf"), **f64)], -1)
        self._food_dist_min = size[adv:, None] + _FOOD_SIZE                                # [G, 1]
        self._forest_dist_min = size[:, None] + _FOREST_SIZE                               # [A, 1]
        self._max_speed = torch.tensor([_MAX_SPEED[k] for k in kind], **f64).view(1, a, 1)
        self._good_others = self._others[adv:, adv:]                                       # [G, G]
        self._leader = torch.arange(a, device=self.device).view(a, 1) == 0                 # [A, 1]
        self._word_ids = torch.arange(_WORDS, dtype=torch.int64, device=self.device)

    def agent_obs(self, obs, agent_id):
        """Agent ``agent_id``'s own observation: a column view of the rows ``step`` / ``reset`` return."""
        lo = sum(self.obs_dims[:agent_id])
        return obs[..., lo:lo + self.obs_dims[agent_id]]

    def _obs_shape(self):
        return (self.n, sum(self.obs_dims))

    @property
    def graph_safe(self):
        return (self.device.type == "cuda" and self.a <= KERNEL_MAX_AGENTS
                and self.num_obstacles <= KERNEL_MAX_LANDMARKS)

    def _restart(self, which, fresh):
        torch = self._torch
        super()._restart(which, fresh)
        self.comm = torch.where(which, torch.full_like(self.comm, -1), self.comm)

    def inside(self):
        """-> bool [N, A, 2]: agent i is inside forest f (simple_world_comm.py:235-238 is_collision)."""
        forests = self.landmarks[:, self.num_obstacles + _FOOD:]
        delta = self.pos[:, :, None, :] - forests[:, None, :, :]
        return self._torch.sqrt((delta ** 2).sum(-1)) < self._forest_dist_min

    def visible(self, inside=None):
        """-> bool [N, A, A]: agent i sees agent j (simple_world_comm.py:253-255)."""
        inside = self.inside() if inside is None else inside
        together = (inside[:, :, None, :] & inside[:, None, :, :]).any(-1)
        open_ = ~inside.any(-1)
        return self._leader | together | (open_[:, :, None] & open_[:, None, :])

    def _obs(self):
        torch = self._torch
        n, a, l, adv = self.n, self.a, self.l, self.num_adversaries
        good = a - adv
        inside = self.inside()
        seen = self.visible(inside)[..., None]                                             # [n, i, j, 1]
        rel_land = (self.landmarks[:, None, :, :] - self.pos[:, :, None, :]).reshape(n, a, 2 * l)
        rel_other = self.pos[:, None, :, :] - self.pos[:, :, None, :]                      # [n, i, j] = pos_j - pos_i
        rel_other = torch.where(seen, rel_other, torch.zeros_like(rel_other))
        rel_other = rel_other[:, self._others].reshape(n, a, 2 * (a - 1))
        good_vel = self.vel[:, None, adv:, :].expand(n, a, good, 2)                        # [n, i, g] = vel_g
        good_vel = torch.where(seen[:, :, adv:], good_vel, torch.zeros_like(good_vel))
        in_forest = torch.where(inside, 1.0, -1.0).to(torch.float64)                       # [n, a, 2]
        common = torch.cat([self.vel, self.pos, rel_land, rel_other], -1)
        heard = (self.comm[:, None] == self._word_ids).to(torch.float64)[:, None, :].expand(n, adv, _WORDS)
        adversaries = torch.cat([common[:, :adv], good_vel[:, :adv].reshape(n, adv, -1), in_forest[:, :adv], heard], -1)
        others_vel = good_vel[:, adv:][:, self._good_others].reshape(n, good, 2 * (good - 1))
        goods = torch.cat([common[:, adv:], in_forest[:, adv:], others_vel], -1)
        return torch.cat([adversaries.reshape(n, -1), goods.reshape(n, -1)], -1).to(torch.float32)

    def _reward(self):
        torch = self._torch
        adv, food_lo = self.num_adversaries, self.num_obstacles
        delta = self.pos[:, adv:, None, :] - self.pos[:, None, :adv, :]                    # [N, G, Nadv, 2]
        dist = torch.sqrt((delta ** 2).sum(-1))
        caught = dist < self._dist_min[adv:, :adv]
        hits = caught.sum((1, 2)).to(torch.float64)                                        # every pair, for every adversary
        adversaries = -0.1 * dist.min(1).values + _CATCH * hits[:, None]
        # the screen's edge (simple_world_comm.py:166-175): 0 below 0.9, a ramp to 1 at 1.0, then exp(2 x - 2) up to 10
        x = self.pos[:, adv:].abs()
        bound = torch.where(x < 0.9, torch.zeros_like(x),
                            torch.where(x < 1.0, (x - 0.9) * 10, torch.exp(2 * x - 2).clamp(max=10.0)))
        to_food = self.pos[:, adv:, None, :] - self.landmarks[:, None, food_lo:food_lo + _FOOD, :]
        to_food = torch.sqrt((to_food ** 2).sum(-1))                                       # [N, G, 2]
        fed = (to_food < self._food_dist_min).sum(2).to(torch.float64)
        good = (-_CATCH * caught.sum(2).to(torch.float64) - 2 * bound.sum(-1) + _FOOD_REWARD * fed
                + 0.05 * to_food.min(2).values)
        return torch.cat([adversaries, good], -1)

    def _indices(self, actions):
        """-> (movement indices [N, A], the leader's word [N]) from index actions [N, A + 1] (movement, word, the others'
        movements) or concatenated one-hots [N, 9 + 5 (A - 1)]."""
        torch = self._torch
        lead = _MOVES + _WORDS
        if actions.shape == (self.n, lead + _MOVES * (self.a - 1)):                        # one-hot (the host protocol)
            moves = torch.cat([actions[:, :_MOVES].argmax(-1, keepdim=True),
                               actions[:, lead:].reshape(self.n, self.a - 1, _MOVES).argmax(-1)], -1)
            return moves, actions[:, _MOVES:lead].argmax(-1)
        assert actions.shape == (self.n, self.a + 1), tuple(actions.shape)
        idx = actions.to(torch.int64)
        return torch.cat([idx[:, :1], idx[:, 2:]], -1), idx[:, 1]

    def _forces(self, actions):
        moves, word = self._indices(actions)
        self.comm = word.clone()                # the word becomes the communication state (core.py:280-288)
        return (self._action_forces(moves) + self._contact_forces(self._dist_min)
                + self._landmark_contact_forces(self._landmark_dist_min))

    def _kernel_actions(self, actions):
        if actions.shape == (self.n, self.a + 1):
            return actions
        moves, word = self._indices(actions)
        return self._torch.cat([moves[:, :1], word[:, None], moves[:, 1:]], -1)

    def _launch(self, idx, fresh, obs, rewards, dones, per_agent):
        from onpolicy import _native
        p = _native.ptr
        fresh_pos, fresh_land = fresh or (None, None)
        _native.check(_native.lib().mappo_simple_world_comm_step(
            p(self.pos), p(self.vel), p(self.landmarks), p(self.t), p(self.comm), p(idx), p(fresh_pos), p(fresh_land),
            p(obs), p(rewards), p(dones), p(per_agent), self.n, self.a, self.num_adversaries, self.num_obstacles,
            self.world_length, int(self.auto_reset), _native.stream_of(self.device)), "mappo_simple_world_comm_step")
