"""Runner for turn-based Hanabi (``train_hanabi_forward.py``).  Interface of the reference's
onpolicy/runner/shared/hanabi_runner_forward.py (HanabiRunner: run :20, warmup :125, collect :138,
train :222, eval :229).

The reference keeps the bookkeeping of a turn in a dozen numpy arrays shaped like a buffer row and re-uploads all of
them with every ``chooseinsert``.  Here the turn state lives on the policy's device (``_TurnState``: one tensor per
buffer field, [N, A, ...]): ``chooseinsert`` is a device-to-device slab write (K2), the reward shift before each update
(reference :59-63) device copies, ``compute`` / ``train`` the GAE kernel and the fused update.  How a buffer step's A
moves are played is the business of ``self.route``, chosen once in ``__init__`` (runner/shared/hanabi_routes.py: host
tables, device tables, device turns); what follows an env step stands once, in runner/shared/hanabi_turns.py.
Evaluation plays on the host stepper move by move (``_eval_games``) or, with ``--use_device_eval``, on device-resident eval
tables without the host (runner/shared/hanabi_eval.py: K18, captured moves).
"""
import os
import time

import numpy as np
import torch

from onpolicy.runner.shared import hanabi_routes
from onpolicy.runner.shared.base_runner import Runner, _t2n


class _TurnState(object):
    """Per-thread data of the turn in progress, shaped like one buffer row [N, A, ...], on ``device``."""

    def __init__(self, n, buffer, device):
        z = lambda t: torch.zeros((n,) + tuple(t.shape[2:]), dtype=torch.float32, device=device)
        o = lambda t: torch.ones((n,) + tuple(t.shape[2:]), dtype=torch.float32, device=device)
        self.obs, self.share_obs = z(buffer.obs), z(buffer.share_obs)
        self.available_actions = z(buffer.available_actions)
        self.values, self.actions = z(buffer.value_preds), z(buffer.actions)
        self.action_log_probs = z(buffer.action_log_probs)
        self.rnn_states, self.rnn_states_critic = z(buffer.rnn_states), z(buffer.rnn_states_critic)
        self.masks, self.active_masks, self.bad_masks = o(buffer.masks), o(buffer.masks), o(buffer.masks)
        self.rewards = z(buffer.rewards)
        self.rewards_since_last_action = z(buffer.rewards)


class HanabiRunner(Runner):
    def __init__(self, config):
        super(HanabiRunner, self).__init__(config)
        self.true_total_num_steps = 0
        route = hanabi_routes.HostTables
        if getattr(self.envs, "device_resident", False):
            route = hanabi_routes.DeviceTables
            if getattr(self.all_args, "use_device_turns", False):
                why = self._device_turns_refusal()
                if why:
                    print("device turns: %s; the rollout stays on the default device route" % why)
                else:
                    route = hanabi_routes.DeviceTurns
        self.route = route(self)
        # opt-in (--use_device_eval): the evaluation plays on device-resident eval tables without the host (hanabi_eval.py)
        self.device_eval = None
        if getattr(self.all_args, "use_device_eval", False) and getattr(self.eval_envs, "device_resident", False):
            from onpolicy.runner.shared import hanabi_eval
            self.device_eval = hanabi_eval.DeviceEval(self)

    def _device_turns_refusal(self):
        """Why this runner cannot take the host-free route (None: it can).  A recurrent policy takes it with a second opt-in
        (``--use_device_turns_rnn``: the moves then keep its two RNN states, hanabi_turns.py)."""
        from onpolicy.algorithms.utils import distributions
        args, space = self.all_args, self.envs.action_space[0]
        if hanabi_routes.recurrent_policy(args) and not getattr(args, "use_device_turns_rnn", False):
            return "a recurrent policy carries per-table state through the moves"
        if distributions.SAMPLING_RNG != "device":
            return "--sampler_rng host draws on the CPU generator"
        if space.__class__.__name__ != "Discrete" or space.n > 64 or os.environ.get("MAPPO_FUSED_SAMPLE", "1") == "0":
            return "the action head is not one the device sampler (K14) takes"
        return None

    # what callers read on the runner: the route's
    scores = property(lambda self: self.route.scores)
    turn_graphs = property(lambda self: self.route.turn_graphs)
    use_obs = property(lambda self: self.route.use_obs)
    use_share_obs = property(lambda self: self.route.use_share_obs)
    use_available_actions = property(lambda self: self.route.use_available_actions)

    def begin_rollout(self):
        """Turn state and the first deal: what run() sets up before its first buffer step."""
        self.turn = _TurnState(self.n_rollout_threads, self.buffer, self.buffer.device)
        self.warmup()

    def warmup(self):
        self.route.warmup()

    def collect(self, step):
        return self.route.collect(step)

    def read_turn_counters(self):
        return self.route.score_summary()

    def insert_and_restart(self):
        """The turn just played -> the buffer; then new games on the tables ``collect`` marked, their rows merged in."""
        b, turn = self.buffer, self.turn
        b.chooseinsert(turn.share_obs, turn.obs, turn.rnn_states, turn.rnn_states_critic, turn.actions,
                       turn.action_log_probs, turn.values, turn.rewards, turn.masks, turn.bad_masks,
                       turn.active_masks, turn.available_actions)
        self.route.restart()

    def run(self):
        self.begin_rollout()
        start = time.time()
        episodes = int(self.num_env_steps) // self.episode_length // self.n_rollout_threads_job
        T = self.episode_length
        b, turn = self.buffer, self.turn
        train_infos = {}
        for episode in range(episodes):
            if self.use_linear_lr_decay:
                self.trainer.policy.lr_decay(episode, episodes)
            self.route.begin_episode()
            for step in range(T):
                self.collect(step)

                if step == 0 and episode > 0:
                    # the last buffer row gets the turn that has just been played ...
                    b.share_obs[-1] = turn.share_obs
                    b.obs[-1] = turn.obs
                    b.available_actions[-1] = turn.available_actions
                    b.active_masks[-1] = turn.active_masks
                    # ... and every reward moves one step earlier (it is only known a turn later)
                    b.rewards[0:T - 1] = b.rewards[1:].clone()
                    b.rewards[-1] = turn.rewards
                    self.compute()
                    train_infos = self.train()

                self.insert_and_restart()

            total_num_steps = (episode + 1) * T * self.n_rollout_threads_job
            if episode % self.save_interval == 0 or episode == episodes - 1:
                self.save()
            if episode % self.log_interval == 0 and episode > 0:
                end = time.time()
                print("\n Env {} Algo {} Exp {} updates {}/{} episodes, total num timesteps {}/{}, FPS {}.\n"
                      .format(getattr(self.all_args, "hanabi_name", "?"), self.algorithm_name, self.experiment_name,
                              episode, episodes, total_num_steps, self.num_env_steps,
                              int(total_num_steps / (end - start))))
                if self.env_name == "Hanabi":
                    average_score = self.route.score_summary()["average_score"]
                    print("average score is {}.".format(average_score))
                    self._log_scalar('average_score', average_score, self.true_total_num_steps)
                train_infos["average_step_rewards"] = float(b.rewards.mean())
                self.log_train(train_infos, self.true_total_num_steps)
            if episode % self.eval_interval == 0 and self.use_eval:
                self.route.score_summary()      # brings true_total_num_steps up to date
                self.eval(self.true_total_num_steps)

    def train(self):
        self.trainer.prep_training()
        train_infos = self.trainer.train(self.buffer)
        self.buffer.chooseafter_update()
        return train_infos

    @torch.no_grad()
    def _eval_games(self):
        """Play the eval envs to the end with the deterministic policy -> list of final scores (with ``--use_device_eval``:
        an array, one score per table, from the device route)."""
        if self.device_eval is not None:
            return self.device_eval.games()
        n, envs = self.n_eval_rollout_threads, self.eval_envs
        scores = []
        obs, share_obs, available_actions = envs.reset(np.ones(n, dtype=bool))
        rnn_states = np.zeros((n,) + tuple(self.buffer.rnn_states.shape[2:]), dtype=np.float32)
        masks = np.ones((n, self.num_agents, 1), dtype=np.float32)
        while True:
            for agent_id in range(self.num_agents):
                actions = -np.ones((n, 1), dtype=np.float32)
                choose = np.any(available_actions == 1, axis=1)
                if not np.any(choose):
                    return scores
                self.trainer.prep_rollout()
                action, rnn_state = self.trainer.policy.act(obs[choose], rnn_states[choose, agent_id],
                                                            masks[choose, agent_id], available_actions[choose],
                                                            deterministic=True)
                actions[choose] = _t2n(action)
                rnn_states[choose, agent_id] = _t2n(rnn_state)
                obs, share_obs, rewards, dones, infos, available_actions = envs.step(actions)
                available_actions[np.asarray(dones) == True] = 0.0   # noqa: E712
                for d, info in zip(dones, infos):
                    if d and 'score' in info.keys():
                        scores.append(info['score'])

    @torch.no_grad()
    def eval(self, total_num_steps):
        eval_average_score = np.mean(self._eval_games())
        print("eval average score is {}.".format(eval_average_score))
        self._log_scalar('eval_average_score', eval_average_score, total_num_steps)

    @torch.no_grad()
    def eval_100k(self, eval_games=100000):
        scores = []
        for trial in range(int(eval_games / self.n_eval_rollout_threads)):
            print("trail is {}".format(trial))
            scores.extend(self._eval_games())
        eval_average_score = np.mean(scores)
        print("eval average score is {}.".format(eval_average_score))
        return eval_average_score
