"""What a host-free Hanabi move is made of, once, for the routes that play such moves: the training route "device turns"
(``hanabi_routes.DeviceTurns``, K17: runner/shared/hanabi_turns.py) and the device evaluation (``hanabi_eval.DeviceEval``,
K18: runner/shared/hanabi_eval.py).

Operands (``MoveOperands``): who can move, the env's actions and the per-table counters, the latter packed into one block
that the host reads back in ONE copy.  Launching (``launch``): the route's descriptor with the call's dynamic pointers bound,
one entry point of libmappo_hip.so.  ``raise_if_refused``: what a read-back counter block says about illegal moves.

The captured move (``MoveGraph``, ``build``).  A move -- ``route.move(a)`` -- is launches only: the policy's forward on all N
rows of the static current-row tensors, K14's draw (training) or its deterministic action (evaluation), the route's ``begin``
operation, the env's apply + deal and encode (K16), the route's ``end`` operation.  Nothing in it depends on the host, and the
move of agent index ``a`` runs the same kernels on the same addresses every time (``a`` is a kernel argument and selects the
slot of the turn tensors / of the carried RNN states), so each of the A <= 5 moves is captured once -- one graph per agent
index -- with the machinery of rollout_graph.py: warm-up on a side stream, ``capturing()``, snapshot and restore of
everything the move advances (the tables with their generators -- they have no ``torch.Generator``, so nothing goes through
``register_generator_state`` -- the env's row tensors, the route's operands ``route.ops.state_tensors()``, torch's device
generator), the pointer-stability check, ``captured()``'s fall-back.  Building the graphs does not show in what is played
(tests/test_gpu_hanabi_turns.py and tests/test_gpu_hanabi_eval.py compare captured and eager runs bit for bit).  The two
routes differ in two things.  The training move runs the critic, so a PopArt head is read through static copies that
every ``begin_episode`` refreshes (``with_value_head``); the evaluation move never runs the critic.  And each keeps its own
switch: ``MAPPO_TURN_GRAPH=0`` / ``MAPPO_EVAL_GRAPH=0`` (the switch of eval_graph.py) keeps the route's eager loop; so
does a capture that fails, with ``captured()``'s message.
"""
import ctypes
import os

import numpy as np
import torch

from onpolicy import _native
from onpolicy.envs.hanabi.device import REFUSED_MOVE
from onpolicy.runner.shared import rollout_graph


class MoveOperands(object):
    """What every host-free move reads and writes besides the policy's and the env's outputs and the route's own tensors:
    who can move and the env's actions [N], and the per-table counters the subclass names in ``COUNTERS`` (name, dtype), each
    an attribute [N].  A subclass adds its tensors, ``state_tensors()`` and ``_describe()`` (its descriptor, checked)."""

    COUNTERS = ()

    def __init__(self, n, players, device):
        self.n, self.players, self.device = int(n), int(players), device
        self.can_move = torch.zeros(n, dtype=torch.int32, device=device)
        self.env_actions = torch.full((n,), -1, dtype=torch.int32, device=device)
        # the counters share one allocation: the host reads them back in ONE copy (``read_counters``).  The kernels take
        # every counter aligned to its own element size, which falling element sizes in ``COUNTERS`` give for every n
        self._spans, at = {}, 0
        for name, dt in self.COUNTERS:
            size = torch.empty((), dtype=dt).element_size()
            if at % size:
                raise ValueError("%s.COUNTERS: %s (%s) would start at byte %d of the block with %d tables; order the "
                                 "counters by falling element size" % (type(self).__name__, name, dt, at, n))
            self._spans[name] = (at, at + n * size, dt)
            at += n * size
        self.counter_block = torch.zeros(at, dtype=torch.uint8, device=device)
        for name, (a, b, dt) in self._spans.items():
            setattr(self, name, self.counter_block[a:b].view(dt))
        self._desc = None

    def read_counters(self):
        """ONE device -> host copy -> {counter name: numpy array [N]}."""
        host = self.counter_block.cpu()
        return {name: host[a:b].view(dt).numpy() for name, (a, b, dt) in self._spans.items()}

    def descriptor(self):
        """The route's C struct with every static pointer filled in (built and checked once, on the first launch)."""
        if self._desc is None:
            d = self._describe()
            for name in ("can_move", "env_actions") + tuple(name for name, _ in self.COUNTERS):
                setattr(d, name, getattr(self, name).data_ptr())
            d.n_tables, d.players = self.n, self.players
            self._desc = d
        return self._desc


def raise_if_refused(counters):
    """counters: what ``read_counters`` returned.  A table that refused a move is an error of the caller's."""
    if counters["refused"].any():
        raise ValueError(REFUSED_MOVE % int(np.flatnonzero(counters["refused"])[0]))


# ------------------------------------------------------------------------------------------- launching
def use_kernels(tensor):
    return tensor.is_cuda and os.environ.get("MAPPO_TURN_KERNELS", "1") != "0"


def flat(t, n, dtype, what):
    if t.dtype != dtype or t.numel() != n:
        raise ValueError("%s: expected %d values of %s, got %s of %s" % (what, n, dtype, tuple(t.shape), t.dtype))
    return t.contiguous()


def launch(o, entry, agent, **dynamic):
    """``entry`` of libmappo_hip.so on ``o.descriptor()`` for agent index ``agent``.  dynamic: the pointers of this call,
    descriptor field -> (tensor, numel, dtype)."""
    d = o.descriptor()
    keep = []       # (a contiguous temporary lives until the call has been enqueued)
    for name, (t, numel, dtype) in dynamic.items():
        t = flat(t, numel, dtype, name)
        keep.append(t)
        setattr(d, name, t.data_ptr())
    with torch.cuda.device(o.device):
        _native.check(getattr(_native.lib(), entry)(ctypes.byref(d), int(agent), _native.stream_of(o.device)), entry)


# ------------------------------------------------------------------------------------------- the captured move
class MoveGraph(rollout_graph.RolloutGraph):
    """The move of agent index ``agent`` on ``route``, which plays on ``envs`` (``n_rows`` tables)."""

    def __init__(self, runner, route, agent, envs, n_rows, device, with_value_head):
        self._init_common(runner, device)
        self.envs, self.N = envs, n_rows
        self.route, self.agent = route, agent
        if with_value_head:
            self._init_head(runner)

    @torch.no_grad()
    def _body(self):
        self.route.move(self.agent)
        return None, None

    def _carried(self):
        return self.route.ops.state_tensors()

    def begin_episode(self):
        """Nothing is carried in tensors of the graph's own: the route's operands are the static tensors.  A PopArt head is
        read through static copies, as the last train() left it."""
        if self.popart is not None:
            self.v_w.copy_(self.popart.weight.data)
            self.v_b.copy_(self.popart.bias.data)

    def step(self):
        self.graph.replay()
        self.replays += 1


class MoveGraphs(object):
    """The A captured moves of a route, by agent index."""

    def __init__(self, graphs):
        self.graphs = graphs

    def __iter__(self):
        return iter(self.graphs)

    def __getitem__(self, agent):
        return self.graphs[agent]

    @property
    def replays(self):
        return sum(g.replays for g in self.graphs)

    def buffer_step(self):
        for g in self.graphs:
            g.begin_episode()
            g.step()


def build(runner, route, envs, n_rows, device, with_value_head, enabled, what):
    """-> the captured moves of ``route`` (all A of them), or None when it has to stay on its eager loop: its switch is off
    (``enabled``), no HIP device, tables that cannot be captured, or a capture that failed (``what`` names the move in
    ``captured()``'s message).  The tables are as the route left them: the capture puts them back."""
    dev = torch.device(device)
    if not enabled or dev.type != "cuda" or not getattr(envs, "graph_safe", False):
        return None
    graphs = []
    for agent in range(runner.num_agents):
        g = rollout_graph.captured(lambda: MoveGraph(runner, route, agent, envs, n_rows, dev, with_value_head), dev, what=what)
        if g is None:
            return None
        graphs.append(g)
    return MoveGraphs(graphs)
