"""What the multi-agent particle scenarios share: the physics constants (reference onpolicy/envs/mpe/core.py), the lazy
``infos`` of the device-resident envs, and ``TorchParticleWorlds``, the base class of worlds held as tensors on the
policy's device.  A scenario (simple_spread.py, simple_reference.py,
simple_speaker_listener.py, simple_push.py, simple_tag.py, simple_world_comm.py) adds its spaces, its extra state, its forces, reward and observation, and the one native call
that is its step on a HIP device.
"""
DT = 0.1
DAMPING = 0.25
SENSITIVITY = 5.0
CONTACT_FORCE = 1e2
CONTACT_MARGIN = 1e-3
AGENT_SIZE = 0.15


class _LazyInfos(object):
    """``infos[i][j]['individual_reward']`` of the reference protocol, materialised from the device only if somebody
    looks (the runner reads the last step's infos once per log interval)."""

    def __init__(self, per_agent):
        self._per_agent, self._rows = per_agent, None

    def fresh(self):
        """A view of the same per-agent tensor that has materialised nothing yet (a replayed graph rewrites the tensor)."""
        return _LazyInfos(self._per_agent)

    def _materialise(self):
        if self._rows is None:
            self._rows = [[{"individual_reward": float(v)} for v in row] for row in self._per_agent.cpu().tolist()]
        return self._rows

    def __len__(self):
        return self._per_agent.shape[0]

    def __iter__(self):
        return iter(self._materialise())

    def __getitem__(self, i):
        return self._materialise()[i]


class TorchParticleWorlds(object):
    """``n_threads`` particle worlds of ``a`` agents and ``l`` landmarks as tensors on ``device``.  State is float64 like
    the reference's numpy physics: pos / vel [N, A, 2], landmarks [N, L, 2], t [N] and whatever the scenario adds;
    observations and rewards leave as float32.

    ``device_resident = True`` tells the runner to hand over the integer action tensor as it comes out of the policy
    (the host protocol's one-hot arrays are accepted as well) and to expect tensors back: obs [N, A, Do] float32,
    rewards [N, A, 1] float32, dones [N, A] bool, infos (lazy).  On a HIP device a step is one launch (K11 family) that
    advances the state in place; ``_step_ops`` is the same step as tensor operations (any device, ~60 small launches)
    and consumes the same generator draws.

    A scenario supplies ``_fresh``, ``_forces``, ``_reward``, ``_obs``, ``_kernel_actions`` and ``_launch``; one with
    state of its own extends ``state_names`` and ``_restart``.  One whose agents observe vectors of different widths
    passes the widths as a tuple for ``obs_dim`` (kept per agent in ``obs_dims``) and overrides ``_obs_shape``;
    one with agents that do not move sets ``_movable``; one that is not collaborative (environment.py:49-50, :140-143) clears
    ``shared_reward`` and pays every agent its own reward instead of the agents' sum; one whose agents differ in
    acceleration passes ``action_scale`` per agent, and one whose agents have a top speed (core.py:272-277) sets
    ``_max_speed``."""
    device_resident = True
    shared_reward = True        # every agent is paid the sum of the agents' rewards (world.collaborative)
    # the tensors a captured rollout graph snapshots / restores and expects to stay in place (runner/shared/rollout_graph.py)
    state_names = ("pos", "vel", "landmarks", "t")
    landmark_scale = 1.0        # restarted landmarks lie at landmark_scale * U(-1, 1)
    _movable = None             # bool [1, A, 1] where some agents are not integrated (core.py:162); None: all move
    _max_speed = None           # float64 [1, A, 1], each agent's top speed (core.py:272-277); None: no clamp

    def __init__(self, n_threads, num_agents, num_landmarks, episode_length, seed, auto_reset, device, obs_dim,
                 action_space, action_scale=SENSITIVITY):
        import torch
        self._torch = torch
        self.auto_reset = auto_reset      # finished worlds restart inside step(), as the vec-env workers do
        self.device = torch.device(device)
        self.n, self.a, self.l = int(n_threads), int(num_agents), int(num_landmarks)
        self.world_length = int(episode_length)
        self.rng = torch.Generator(device=self.device)
        self.rng.manual_seed(int(seed))
        from onpolicy.envs.spaces import Box
        # observation width per agent; ``obs_dim`` only where all agents share one
        dims = self.obs_dims = tuple(obs_dim) if isinstance(obs_dim, (tuple, list)) else (obs_dim,) * self.a
        assert len(dims) == self.a, dims
        if len(set(dims)) == 1:
            self.obs_dim = dims[0]
        self.observation_space = [Box(shape=(d,)) for d in dims]
        self.share_observation_space = [Box(shape=(sum(dims),)) for _ in range(self.a)]
        self.action_space = [action_space() for _ in range(self.a)] if callable(action_space) else list(action_space)
        f64 = dict(dtype=torch.float64, device=self.device)
        self.pos = torch.zeros(self.n, self.a, 2, **f64)
        self.vel = torch.zeros(self.n, self.a, 2, **f64)
        self.landmarks = torch.zeros(self.n, self.l, 2, **f64)
        self.t = torch.zeros(self.n, dtype=torch.int64, device=self.device)
        # action index -> force direction (environment.py: u[0] += a[1] - a[2], u[1] += a[3] - a[4])
        # times the action scale: the sensitivity, or one scale per agent ([A, 5, 2] then, see ``_action_forces``)
        self._directions = torch.tensor([[0, 0], [1, 0], [-1, 0], [0, 1], [0, -1]], **f64)
        if isinstance(action_scale, (tuple, list)):
            assert len(action_scale) == self.a, action_scale
            self._directions = torch.tensor(action_scale, **f64).view(self.a, 1, 1) * self._directions
        else:
            self._directions = self._directions * action_scale

    def _uniform(self, *shape):
        torch = self._torch
        # U(-1, 1) in one launch: uniform_ evaluates rand * (to - from) + from on the same draws as torch.rand
        return torch.empty(*shape, dtype=torch.float64, device=self.device).uniform_(-1.0, 1.0, generator=self.rng)

    # -- random draws: the same calls, in the same order, on both step paths
    def _fresh(self):
        """Reset draws for every world, in the order the native step takes them: agent positions, landmarks, ..."""
        return self._uniform(self.n, self.a, 2), self._uniform(self.n, self.l, 2)

    def _restart(self, which, fresh):
        """Branch-free (no host sync): ``fresh`` is drawn for every world and kept where ``which`` is set."""
        torch = self._torch
        w = which.view(-1, 1, 1)
        self.pos = torch.where(w, fresh[0], self.pos)
        self.vel = torch.where(w, torch.zeros_like(self.vel), self.vel)
        self.landmarks = torch.where(w, self.landmark_scale * fresh[1], self.landmarks)
        self.t = torch.where(which, torch.zeros_like(self.t), self.t)

    def _action_forces(self, idx):
        """Movement indices [N, A] -> the action force on each agent [N, A, 2] where the action scale is per agent."""
        return self._directions[self._torch.arange(self.a, device=self.device), idx]

    def _contact_forces(self, dist_min):
        """Soft contacts between agents closer than ``dist_min``, the sum of their radii (core.py:290-321; a scalar, or
        [A, A] where the radii differ) -> the force on each agent [N, A, 2].  Coincident agents exert none (the
        reference divides by zero there).  Needs ``self._others``, the [A, A] mask without its diagonal."""
        torch = self._torch
        delta = self.pos[:, :, None, :] - self.pos[:, None, :, :]
        dist = torch.sqrt((delta ** 2).sum(-1))
        pen = torch.logaddexp(torch.zeros_like(dist), -(dist - dist_min) / CONTACT_MARGIN) * CONTACT_MARGIN
        f = CONTACT_FORCE * delta / dist[..., None] * pen[..., None]
        f = torch.where(self._others[None, :, :, None], f, torch.zeros_like(f))       # no self force (0 / 0 there)
        return torch.nan_to_num(f, nan=0.0, posinf=0.0, neginf=0.0).sum(2)

    def _landmark_contact_forces(self, dist_min):
        """Soft contacts between agents and landmarks that collide and do not move (core.py:318-320): ``dist_min`` is the
        sum of the two radii, a scalar or [A, 1] per agent -> the force on each agent [N, A, 2], away from the landmark.
        An agent on a landmark's centre takes none, as with coincident agents."""
        torch = self._torch
        delta = self.pos[:, :, None, :] - self.landmarks[:, None, :, :]
        dist = torch.sqrt((delta ** 2).sum(-1))
        pen = torch.logaddexp(torch.zeros_like(dist), -(dist - dist_min) / CONTACT_MARGIN) * CONTACT_MARGIN
        f = CONTACT_FORCE * delta / dist[..., None] * pen[..., None]
        return torch.nan_to_num(f, nan=0.0, posinf=0.0, neginf=0.0).sum(2)

    def reset(self):
        self._restart(self._torch.ones(self.n, dtype=self._torch.bool, device=self.device), self._fresh())
        return self._obs()

    def reset_in_place(self):
        """``reset()`` -- the same generator draws in the same order, the same state and observations bit for bit -- with
        every tensor named by ``state_names`` kept at its address (``reset`` rebinds them): what a captured graph that
        holds those addresses needs of a reset between its replays (runner/shared/eval_graph.py)."""
        kept = {name: getattr(self, name) for name in self.state_names}
        self._restart(self._torch.ones(self.n, dtype=self._torch.bool, device=self.device), self._fresh())
        for name, tensor in kept.items():
            tensor.copy_(getattr(self, name))
            setattr(self, name, tensor)
        return self._obs()

    @property
    def graph_safe(self):
        """True when ``step`` advances the state tensors IN PLACE (the kernel path): a captured rollout graph
        (runner/shared/rollout_graph.py) may then replay it.  The tensor-op path rebinds them."""
        return self.device.type == "cuda"

    def step(self, actions):
        actions = self._torch.as_tensor(actions, device=self.device)
        return self._step_kernel(actions) if self.graph_safe else self._step_ops(actions)

    def _obs_shape(self):
        """The shape observations leave ``step`` / ``reset`` in: [N, A, Do] where the agents share one width (a scenario
        whose ``obs_dims`` differ has no ``obs_dim`` and lays its rows out itself)."""
        return (self.n, self.a, self.obs_dim)

    def _step_kernel(self, actions):
        """The whole step as one launch: the arithmetic and the generator draws of ``_step_ops``."""
        torch = self._torch
        idx = self._kernel_actions(actions).to(torch.int64).contiguous()
        fresh = self._fresh() if self.auto_reset else None
        obs = torch.empty(self._obs_shape(), dtype=torch.float32, device=self.device)
        rewards = torch.empty(self.n, self.a, 1, dtype=torch.float32, device=self.device)
        dones = torch.empty(self.n, self.a, dtype=torch.bool, device=self.device)
        per_agent = torch.empty(self.n, self.a, dtype=torch.float64, device=self.device)
        for name in self.state_names:
            setattr(self, name, getattr(self, name).contiguous())
        self._launch(idx, fresh, obs, rewards, dones, per_agent)
        return obs, rewards, dones, _LazyInfos(per_agent)

    def _step_ops(self, actions):
        torch = self._torch
        force = self._forces(actions)
        # core.py:265-278: damping, then force * dt (every mass is 1), then the top speed where agents have one
        vel = self.vel * (1 - DAMPING) + force * DT
        if self._max_speed is not None:
            speed = torch.sqrt(vel[..., 0:1] ** 2 + vel[..., 1:2] ** 2)
            vel = torch.where(speed > self._max_speed, vel / speed * self._max_speed, vel)
        pos = self.pos + vel * DT
        if self._movable is not None:
            vel, pos = torch.where(self._movable, vel, self.vel), torch.where(self._movable, pos, self.pos)
        self.vel, self.pos = vel, pos
        self.t = self.t + 1
        per_agent = self._reward()
        if self.shared_reward:
            rewards = per_agent.sum(-1, keepdim=True).expand(self.n, self.a).unsqueeze(-1).to(torch.float32)
        else:
            rewards = per_agent[..., None].to(torch.float32)
        done_env = self.t >= self.world_length
        dones = done_env[:, None].expand(self.n, self.a)
        if self.auto_reset:
            self._restart(done_env, self._fresh())
        return self._obs(), rewards, dones, _LazyInfos(per_agent)

    def close(self):
        pass
