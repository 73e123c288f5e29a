"""One player's move of the Hanabi device evaluation (``--use_device_eval``) as ONE graph launch, one graph per agent index.

On that route (``hanabi_eval.DeviceEval``) a move -- ``route.move(a)`` -- is launches only: the actor's forward on all N rows
of the static current-row tensors, its deterministic action (K14 mode), ``eval_begin`` (K18), the env's apply + deal and
encode (K16), ``eval_end`` (K18).  Nothing in it depends on the host, and the move of agent index ``a`` runs the same kernels on
the same addresses every round (``a`` is a kernel argument and selects the slot of the carried RNN states), so each of the
A <= 5 moves is captured once, on the first evaluation, with the machinery of rollout_graph.py: warm-up on a side stream,
``capturing()``, snapshot and restore of everything the move advances (the eval tables with their generators -- they have no
``torch.Generator`` -- the env's row tensors and the route's operands, torch's device generator), the pointer-stability
check, ``captured()``'s fall-back.  The critic is not run, so no PopArt head is involved, and everything is recorded on one
stream.  Building the graphs does not show in the games (tests/test_gpu_hanabi_eval.py compares captured and eager
evaluations bit for bit).

``MAPPO_EVAL_GRAPH=0`` (the switch of eval_graph.py) keeps the route's eager loop; so does a capture that fails, with
``captured()``'s message.
"""
import torch

from onpolicy.runner.shared import eval_graph, rollout_graph


class HanabiEvalGraph(rollout_graph.RolloutGraph):
    """The evaluation move of agent index ``agent``."""

    def __init__(self, route, agent):
        runner = route.r
        self._init_common(runner, torch.device(runner.device))
        self.envs = runner.eval_envs
        self.N = runner.n_eval_rollout_threads
        self.route, self.agent = route, agent

    @torch.no_grad()
    def _body(self):
        self.route.move(self.agent)
        return None, None

    def _carried(self):
        return self.route.ops.state_tensors()

    def begin_episode(self):
        """Nothing is carried in tensors of the graph's own: the route's operands are the static tensors."""

    def step(self):
        self.graph.replay()
        self.replays += 1


def build(route):
    """-> the captured moves of ``route`` (a list, one per agent index), or None when the evaluation stays on its eager
    loop.  Called after the route's ``_begin``: the tables hold freshly dealt games, which the capture puts back."""
    dev = torch.device(route.r.device)
    if not eval_graph.enabled() or dev.type != "cuda" or not getattr(route.envs, "graph_safe", False):
        return None
    graphs = []
    for agent in range(route.players):
        g = rollout_graph.captured(lambda: HanabiEvalGraph(route, agent), dev, what="Hanabi eval move")
        if g is None:
            return None
        graphs.append(g)
    return graphs
