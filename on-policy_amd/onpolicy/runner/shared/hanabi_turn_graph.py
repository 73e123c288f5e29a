"""One player's move of the host-free Hanabi route ("device turns") as ONE graph launch, one graph per agent index.

On that route (``hanabi_routes.DeviceTurns``) a move -- ``route.move(a)`` -- is launches only: the policy's forward on all N
rows of the static current-row tensors, K14's draw, ``turn_begin`` (K17), the env's apply + deal and encode (K16),
``turn_end`` (K17).  Nothing in it depends on the host, and the move of agent index ``a`` runs the same kernels on the same
addresses every buffer step (``a`` is a kernel argument), so each of the A <= 5 moves is captured once, before the first
rollout, with the machinery of rollout_graph.py: warm-up on a side stream, ``capturing()``, snapshot and restore of
everything the move advances (the tables with their generators -- they have no ``torch.Generator`` -- the env's row
tensors, the turn tensors and the route's state, torch's device generator), the pointer-stability check, static copies of a
PopArt head, ``captured()``'s fall-back.  Building the graphs does not show in the trajectories
(tests/test_gpu_hanabi_turns.py compares captured and eager runs bit for bit).

``MAPPO_TURN_GRAPH=0`` keeps the route's eager loop; so does a capture that fails, with ``captured()``'s message.
"""
import os

import torch

from onpolicy.runner.shared import rollout_graph


class HanabiTurnGraph(rollout_graph.RolloutGraph):
    """The move of agent index ``agent``."""

    def __init__(self, runner, agent):
        self._init_common(runner, runner.buffer.device)
        self.agent = agent
        self._init_head(runner)

    @torch.no_grad()
    def _body(self):
        self.r.route.move(self.agent)
        return None, None

    def _carried(self):
        return self.r.route.ops.state_tensors()

    def begin_episode(self):
        """Nothing is carried in tensors of the graph's own; a PopArt head is read through static copies, as the last
        train() left it."""
        if self.popart is not None:
            self.v_w.copy_(self.popart.weight.data)
            self.v_b.copy_(self.popart.bias.data)

    def step(self):
        self.graph.replay()
        self.replays += 1


class HanabiTurnGraphs(object):
    """The A captured moves of a buffer step."""

    def __init__(self, graphs):
        self.graphs = graphs

    @property
    def replays(self):
        return sum(g.replays for g in self.graphs)

    def buffer_step(self):
        for g in self.graphs:
            g.begin_episode()
            g.step()


def enabled():
    return os.environ.get("MAPPO_TURN_GRAPH", "1") != "0"


def build(runner):
    """-> the captured moves of ``runner`` (all A of them), or None when the route has to stay on its eager loop."""
    dev = torch.device(runner.buffer.device)
    if not enabled() or dev.type != "cuda" or not getattr(runner.envs, "graph_safe", False):
        return None
    graphs = []
    for agent in range(runner.num_agents):
        g = rollout_graph.captured(lambda: HanabiTurnGraph(runner, agent), dev, what="Hanabi move")
        if g is None:
            return None
        graphs.append(g)
    return HanabiTurnGraphs(graphs)
