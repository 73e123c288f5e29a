"""One rollout step of the device-resident loop as ONE graph launch.

With the worlds on the GPU (``--use_device_env``: K11) a rollout step of the shared MPE runner -- policy forward of
actor and critic, action sampling, env step, mask / RNN-state bookkeeping (reference
onpolicy/runner/shared/mpe_runner.py:96-139: collect -> envs.step -> insert) -- is ~30 small kernels on a few thousand
rows: pure launch latency (0.75 ms per step at 4096 worlds x 3 agents, five times the update's share of a config-3
iteration).  Nothing in it depends on the host, and every step runs the same kernels on the same buffers except for the
slab of the rollout buffer it writes.  So the step is captured once into a HIP graph that reads and advances a small
carried state (current observation, masks, RNN states) held in static tensors and leaves its results in static output
tensors; a rollout step is then one graph launch + the one fused slab write (K2) into row ``step`` of the buffer, whose
destination pointers are the only thing that changes from step to step.

Random numbers: the action sampler draws from torch's default device generator and the worlds from their own
``torch.Generator``; both are registered with the graph (philox offsets advance with every replay), so a graphed
rollout consumes the same random stream as the eager loop (tests/test_gpu_rollout_graph.py compares whole rollouts).

Falls back to the eager loop (returns None from ``build``) when the step cannot be captured: host envs, worlds whose step
rebinds its state tensors (more than 16 agents / landmarks: the tensor-op path), the integer-parity sampler
(``--sampler_rng host`` draws on the CPU generator), no HIP device.  A PopArt value head is read through static copies that
every ``begin_episode`` refreshes (its ``update`` rebinds the parameters' storage).
"""
import os

import torch

from onpolicy.utils.graph_capture import capturing


class RolloutGraph(object):
    WARMUP = 3

    def _init_common(self, runner, dev):
        """What ``capture`` / ``step`` read whatever the carried state looks like (the separated graph starts here too)."""
        self.r = runner
        self.envs = runner.envs         # the worlds the step advances (the eval graph names the runner's eval worlds)
        self.N, self.A = runner.n_rollout_threads, runner.num_agents
        self.dev = dev
        self.popart = None
        self.graph = None
        self.out = None
        self.infos = None
        self.replays = 0

    def __init__(self, runner):
        b = runner.buffer
        dev = b.device
        self._init_common(runner, dev)
        f32 = dict(dtype=torch.float32, device=dev)
        # carried state of the loop
        self.cur_obs = torch.empty(b.obs.shape[1:], **f32)
        self.cur_masks = torch.empty(b.masks.shape[1:], **f32)
        self.recurrent = b.rnn_states.stride()[0] != 0
        if self.recurrent:
            self.cur_rnn_a = torch.empty(b.rnn_states.shape[1:], **f32)
            self.cur_rnn_c = torch.empty(b.rnn_states_critic.shape[1:], **f32)
        else:       # feed-forward policies: the buffer's zero view serves every step
            self.cur_rnn_a, self.cur_rnn_c = b.rnn_states[0], b.rnn_states_critic[0]
        self.side = torch.cuda.Stream(device=dev)      # the critic's branch of the captured step
        self._init_head(runner)

    def _init_head(self, runner):
        # A PopArt value head REBINDS its weight / bias storage on every update (algorithms/utils/popart.py: the running
        # minibatch's backward still needs the old tensors), so the addresses a capture bakes in would go stale with the first
        # train().  The graph therefore reads static copies of the head, refreshed at the start of every episode.
        head = getattr(runner.trainer.policy.critic, "v_out", None)
        self.popart = head if type(head).__name__ == "PopArt" else None
        if self.popart is not None:
            self.v_w = torch.empty_like(self.popart.weight.data)
            self.v_b = torch.empty_like(self.popart.bias.data)

    # -- the step itself: eager code, captured once
    @torch.no_grad()
    def _body(self):
        r, N, A = self.r, self.N, self.A
        policy = r.trainer.policy
        dev = r.buffer.device
        share = r._share(self.cur_obs, N)
        # The critic's branch (centralised observation -> value) depends on nothing the actor's branch produces, and a
        # forward launch on N * A rows fills a third of the CUs: it is recorded on a side stream, i.e. as a parallel
        # branch of the graph, and runs under the actor forward / sampling / env step of the main branch.
        main = torch.cuda.current_stream(dev)
        self.side.wait_stream(main)
        with torch.cuda.stream(self.side):
            values, rnn_c = policy.critic(r._rows(share), r._rows(self.cur_rnn_c), r._rows(self.cur_masks))
            values, rnn_c = r._per_env(values), r._per_env(rnn_c)
        actions, logp, rnn_a = policy.actor(r._rows(self.cur_obs), r._rows(self.cur_rnn_a), r._rows(self.cur_masks))
        actions, logp, rnn_a = r._per_env(actions), r._per_env(logp), r._per_env(rnn_a)
        obs, rewards, dones, infos = self.envs.step(actions)
        masks = torch.where(dones, 0.0, 1.0).unsqueeze(-1)          # 0 where the episode ended (one launch)
        main.wait_stream(self.side)
        if self.recurrent:
            # finished agents restart from a zero RNN state (reference mpe_runner.py:128-129)
            rnn_a = rnn_a * masks.view(N, A, 1, 1)
            rnn_c = rnn_c * masks.view(N, A, 1, 1)
        # the carried state of the next step
        self.cur_obs.copy_(obs)
        self.cur_masks.copy_(masks)
        if self.recurrent:
            self.cur_rnn_a.copy_(rnn_a)
            self.cur_rnn_c.copy_(rnn_c)
        # (the centralised observation is materialised here, inside the graph, so that the slab write takes it as it is)
        share_next = r._share(obs, N).contiguous() if r.use_centralized_V else obs
        return (share_next, obs, rnn_a, rnn_c, actions, logp, values, rewards, masks), infos

    def _state_names(self):
        """The env's state tensors that a replay advances in place: what the env declares (``state_names``)."""
        return tuple(self.envs.state_names)

    def _env_state(self):
        e = self.envs
        # (an env without ``rng`` keeps its generators inside its state tensors: the Hanabi tables, K16)
        rng = getattr(e, "rng", None)
        return {k: getattr(e, k).clone() for k in self._state_names()}, None if rng is None else rng.get_state(), \
            torch.cuda.get_rng_state(self.dev)

    def _carried(self):
        """The static tensors that carry the loop's state from one replay to the next."""
        return [self.cur_obs, self.cur_masks] + ([self.cur_rnn_a, self.cur_rnn_c] if self.recurrent else [])

    def _prep_rollout(self):
        self.r.trainer.prep_rollout()

    class _StaticHead(object):
        """While active, the PopArt head's parameters live in the graph's static tensors (same values)."""

        def __init__(self, g):
            self.g = g

        def __enter__(self):
            g = self.g
            if g.popart is not None:
                self.saved = (g.popart.weight.data, g.popart.bias.data)
                g.v_w.copy_(self.saved[0])
                g.v_b.copy_(self.saved[1])
                g.popart.weight.data, g.popart.bias.data = g.v_w, g.v_b

        def __exit__(self, *exc):
            g = self.g
            if g.popart is not None:
                g.popart.weight.data, g.popart.bias.data = self.saved

    def _restore(self, snap):
        e = self.envs
        state, env_rng, dev_rng = snap
        for k, v in state.items():
            getattr(e, k).copy_(v)
        if env_rng is not None:
            e.rng.set_state(env_rng)
        torch.cuda.set_rng_state(dev_rng, self.dev)

    def capture(self):
        """Warm the step up on a side stream (library workspaces, lazy module state), capture it, and put worlds and
        generators back where they were: building the graph must not show in the trajectories."""
        r = self.r
        dev = self.dev
        self._prep_rollout()
        self.begin_episode()
        keep = [x.clone() for x in self._carried()]
        snap = self._env_state()
        state_ptrs = {k: getattr(self.envs, k).data_ptr() for k in self._state_names()}
        torch.cuda.synchronize(dev)
        try:        # (warm-up included: whatever fails in here, worlds / generators / carried state go back where they were)
            with self._StaticHead(self):
                side = torch.cuda.Stream(device=dev)
                side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side):
                    for _ in range(self.WARMUP):
                        self._body()
                torch.cuda.current_stream(dev).wait_stream(side)
                torch.cuda.synchronize(dev)
                graph = torch.cuda.CUDAGraph()
                if getattr(self.envs, "rng", None) is not None:
                    graph.register_generator_state(self.envs.rng)
                with capturing(graph):
                    self.out, self.infos = self._body()
                torch.cuda.synchronize(dev)
            # the graph reads and advances the worlds IN PLACE: a step path that rebinds its state tensors cannot be replayed
            moved = [k for k, p in state_ptrs.items() if getattr(self.envs, k).data_ptr() != p]
            if moved:
                raise RuntimeError("env.step rebinds its state tensors (%s): not capturable" % ", ".join(moved))
            self.graph = graph
        finally:
            self._restore(snap)
            for x, kept in zip(self._carried(), keep):
                x.copy_(kept)
        return self

    def begin_episode(self):
        """Row 0 of the buffer is the state the rollout starts from (warmup() / after_update() put it there)."""
        b = self.r.buffer
        self.cur_obs.copy_(b.obs[0])
        self.cur_masks.copy_(b.masks[0])
        if self.recurrent:
            self.cur_rnn_a.copy_(b.rnn_states[0])
            self.cur_rnn_c.copy_(b.rnn_states_critic[0])
        if self.popart is not None:         # the head as the last train() left it
            self.v_w.copy_(self.popart.weight.data)
            self.v_b.copy_(self.popart.bias.data)

    def step(self):
        """One rollout step: graph launch + the fused slab write into the buffer's current row."""
        self.graph.replay()
        self.replays += 1
        self.r.buffer.insert(*self.out)
        # (a fresh lazy view of the static per-agent rewards: the previous one may have cached an older step)
        return self.infos.fresh()


def capturable(envs, device):
    """Whether a rollout step on ``envs`` with the buffers on ``device`` can be captured at all."""
    from onpolicy.algorithms.utils import distributions
    if os.environ.get("MAPPO_ROLLOUT_GRAPH", "1") == "0":
        return False
    # device-resident worlds (envs/mpe/particle_worlds.py) declare ``graph_safe`` (the step advances the tensors named by
    # ``state_names`` in place: the K11 family does) and draw from their own generator ``rng``
    if not getattr(envs, "device_resident", False) or not envs.graph_safe:
        return False
    return torch.device(device).type == "cuda" and distributions.SAMPLING_RNG == "device"


def captured(make, device, what="rollout"):
    """``make().capture()``, or None where that fails: capture is an optimisation, anything it cannot take stays on the
    eager loop."""
    try:
        return make().capture()
    except Exception as exc:
        print("%s graph: capture failed (%s: %s); the %s stays eager" % (what, type(exc).__name__, exc, what))
        try:
            torch.cuda.synchronize(device)
        except Exception:
            pass
        return None


def build(runner):
    """-> a captured RolloutGraph for ``runner``, or None when the step has to stay eager."""
    if not capturable(runner.envs, runner.buffer.device) or getattr(runner, "_mat", False):
        return None
    return captured(lambda: RolloutGraph(runner), runner.buffer.device)
