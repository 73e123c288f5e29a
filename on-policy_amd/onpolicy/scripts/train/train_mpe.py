#!/usr/bin/env python
"""MPE training entry point with the command line of the reference's
onpolicy/scripts/train/train_mpe.py (main :64, parse_args :52-61, env factories :16-49): same flags,
same algorithm-name -> recurrent-flag rewrite, same config dict handed to ``MPERunner``.

Differences: simple_spread comes from the in-tree vectorised implementation (no gym / subprocess workers;
``--use_device_env`` keeps the training worlds on the GPU next to policy and buffer); with ``--use_device_env``
simple_reference comes from the in-tree device implementation as well (envs/mpe/simple_reference.py, shared-policy
runner only), and so does simple_speaker_listener (envs/mpe/simple_speaker_listener.py: two agents with different
spaces, so the separated runner only -- ``--share_policy`` -- with rmappo / mappo / ippo) and simple_push
(envs/mpe/simple_push.py: one adversary and num_agents - 1 good agents with different observations and rewards of their
own, 1 or 2 landmarks; the separated runner only, like simple_speaker_listener) and simple_tag (envs/mpe/simple_tag.py:
``--num_adversaries`` adversaries followed by ``--num_good_agents`` good agents, num_agents their sum; the separated
runner only) and simple_world_comm (envs/mpe/simple_world_comm.py: simple_tag's two kinds of agent among
``--num_landmarks`` obstacles, two pieces of food and two forests that hide agents, the first adversary a leader with a
MultiDiscrete action that says a word per step; 4 adversaries and 2 good agents where the two flags are not given; the
separated runner only); every other case -- simple_reference, simple_speaker_listener, simple_push, simple_tag or
simple_world_comm without the flag, any other scenario, and the eval envs of ``--use_eval`` in every case but one -- is built per worker from an external env tree (MAPPO_ENVS_PATH).  The exception:
``--use_device_eval`` (with ``--use_eval --use_device_env``, rmappo / mappo / ippo) builds the eval worlds of the
device scenarios in-tree on the device too, and ``eval()`` then runs on tensors, its step as one captured graph launch
(runner/shared/eval_graph.py).  wandb / setproctitle are optional.
Example (BASELINE.json configs[0]):
    python -m onpolicy.scripts.train.train_mpe --env_name MPE --scenario_name simple_spread \\
        --num_agents 3 --num_landmarks 3 --n_rollout_threads 8 --episode_length 25 \\
        --num_env_steps 20000 --ppo_epoch 10 --use_ReLU --use_wandb
The reference's train_mpe_reference.sh on the device:
    python -m onpolicy.scripts.train.train_mpe --env_name MPE --algorithm_name rmappo --scenario_name simple_reference \
        --num_agents 2 --num_landmarks 3 --n_rollout_threads 128 --num_mini_batch 1 --episode_length 25 \
        --num_env_steps 3000000 --ppo_epoch 15 --gain 0.01 --lr 7e-4 --critic_lr 7e-4 --use_device_env
The reference's train_mpe_comm.sh on the device (``--share_policy`` is a store_false flag: one policy per agent):
    python -m onpolicy.scripts.train.train_mpe --env_name MPE --algorithm_name rmappo \
        --scenario_name simple_speaker_listener --num_agents 2 --num_landmarks 3 --n_rollout_threads 128 \
        --num_mini_batch 1 --episode_length 25 --num_env_steps 2000000 --ppo_epoch 15 --gain 0.01 --lr 7e-4 \
        --critic_lr 7e-4 --share_policy --use_device_env
Keep-away on the device (an episode is 25 steps whatever --episode_length says, as in the reference):
    python -m onpolicy.scripts.train.train_mpe --env_name MPE --algorithm_name rmappo --scenario_name simple_push \
        --num_agents 2 --num_landmarks 2 --n_rollout_threads 128 --num_mini_batch 1 --episode_length 25 \
        --num_env_steps 2000000 --ppo_epoch 15 --gain 0.01 --lr 7e-4 --critic_lr 7e-4 --share_policy --use_device_env
Predator-prey on the device, three adversaries against one good agent (25-step episodes as well):
    python -m onpolicy.scripts.train.train_mpe --env_name MPE --algorithm_name rmappo --scenario_name simple_tag \
        --num_agents 4 --num_adversaries 3 --num_good_agents 1 --num_landmarks 2 --n_rollout_threads 128 \
        --num_mini_batch 1 --episode_length 25 --num_env_steps 2000000 --ppo_epoch 15 --gain 0.01 --lr 7e-4 \
        --critic_lr 7e-4 --share_policy --use_device_env
Predator-prey with forests, food and a speaking leader on the device, four adversaries against two good agents:
    python -m onpolicy.scripts.train.train_mpe --env_name MPE --algorithm_name rmappo --scenario_name simple_world_comm \
        --num_agents 6 --num_adversaries 4 --num_good_agents 2 --num_landmarks 1 --n_rollout_threads 128 \
        --num_mini_batch 1 --episode_length 25 --num_env_steps 2000000 --ppo_epoch 15 --gain 0.01 --lr 7e-4 \
        --critic_lr 7e-4 --share_policy --use_device_env
"""
import argparse
import sys

from onpolicy.config import get_config
from onpolicy.envs.mpe.simple_push import TorchSimplePush
from onpolicy.envs.mpe.simple_reference import TorchSimpleReference
from onpolicy.envs.mpe.simple_speaker_listener import TorchSimpleSpeakerListener
from onpolicy.envs.mpe.simple_spread import TorchSimpleSpread, VecSimpleSpread
from onpolicy.envs.mpe.simple_tag import TorchSimpleTag
from onpolicy.envs.mpe.simple_world_comm import TorchSimpleWorldComm
from onpolicy.scripts.train import _launch


# scenarios with an in-tree device implementation (--use_device_env; row f1): the worlds are held on the policy's device
DEVICE_ENVS = {"simple_spread": TorchSimpleSpread, "simple_reference": TorchSimpleReference,
               "simple_speaker_listener": TorchSimpleSpeakerListener, "simple_push": TorchSimplePush,
               "simple_tag": TorchSimpleTag, "simple_world_comm": TorchSimpleWorldComm}
# ... of which these run under the separated runner (one policy per agent: the agents' spaces differ), the rest under the shared
SEPARATED_DEVICE_ENVS = ("simple_speaker_listener", "simple_push", "simple_tag", "simple_world_comm")
TAG_DEFAULTS = (3, 1)       # adversaries, good agents where --num_adversaries / --num_good_agents are not given
WORLD_COMM_DEFAULTS = (4, 2)    # ... of simple_world_comm: the reference's documented counts
# the scenarios whose agents are adversaries followed by good agents
KIND_DEFAULTS = {"simple_tag": TAG_DEFAULTS, "simple_world_comm": WORLD_COMM_DEFAULTS}


def tag_counts(all_args):
    """-> (adversaries, good agents) of a simple_tag or simple_world_comm run."""
    adv, good = KIND_DEFAULTS.get(all_args.scenario_name, TAG_DEFAULTS)
    return getattr(all_args, "num_adversaries", adv), getattr(all_args, "num_good_agents", good)


def make_train_env(all_args, n_threads=None, seed_offset=0, device=None):
    n = all_args.n_rollout_threads if n_threads is None else n_threads
    seed_offset += 1000 * getattr(all_args, "rollout_thread_offset", 0)      # data-parallel rank: its own worlds
    if device is not None and all_args.scenario_name in DEVICE_ENVS:
        extra = {"num_adversaries": tag_counts(all_args)[0]} if all_args.scenario_name in KIND_DEFAULTS else {}
        return DEVICE_ENVS[all_args.scenario_name](n, all_args.num_agents, all_args.num_landmarks,
                                                   all_args.episode_length, seed=all_args.seed + seed_offset,
                                                   device=device, **extra)
    if all_args.scenario_name == "simple_spread":       # built in, all worlds advanced by one numpy pass
        return VecSimpleSpread(n, all_args.num_agents, all_args.num_landmarks, all_args.episode_length,
                               seed=all_args.seed + seed_offset)
    # any other scenario: one MPEEnv per worker like the reference (train_mpe.py:16-32); the scenario modules
    # come from an external env tree (MAPPO_ENVS_PATH)
    from onpolicy.envs.env_wrappers import DummyVecEnv, SubprocVecEnv
    from onpolicy.envs.mpe.MPE_env import MPEEnv

    def get_env_fn(rank):
        def init_env():
            env = MPEEnv(all_args)
            env.seed(all_args.seed + seed_offset + rank * 1000)
            return env
        return init_env
    return DummyVecEnv([get_env_fn(0)]) if n == 1 else SubprocVecEnv([get_env_fn(i) for i in range(n)])


def parse_args(args, parser):
    parser.add_argument('--scenario_name', type=str, default='simple_spread', help="Which scenario to run on")
    parser.add_argument("--num_landmarks", type=int, default=3)
    parser.add_argument('--num_agents', type=int, default=2, help="number of players")
    parser.add_argument('--use_device_env', action='store_true', default=False,
                        help="simple_spread or simple_reference (shared-policy runner) or simple_speaker_listener, "
                             "simple_push, simple_tag or simple_world_comm (separated runner: --share_policy) with the training worlds held as "
                             "tensors on the policy's device: no per-step host round trip")
    # (argparse.SUPPRESS: the attribute exists only when the flag is given, so a default parse carries the reference's flags
    # and --use_device_env, nothing else; readers use getattr(args, "fused_multi_loss", False))
    parser.add_argument('--fused_multi_loss', action='store_true', default=argparse.SUPPRESS,
                        help="rmappo / mappo / ippo with a MultiDiscrete action head (simple_reference) on a HIP device: "
                             "the PPO loss of all sub-heads as one kernel launch and the update as a captured graph "
                             "(MAPPO_FUSED_LOSS_MULTI=1 does the same)")
    parser.add_argument('--use_device_eval', action='store_true', default=argparse.SUPPRESS,
                        help="with --use_eval --use_device_env (rmappo / mappo / ippo): the eval worlds are held on the "
                             "policy's device like the training worlds, eval() runs on tensors with the deterministic "
                             "action from one kernel launch, and its step is replayed from a captured graph "
                             "(MAPPO_EVAL_GRAPH=0: the eager tensor loop)")
    # (SUPPRESS as above; the external env tree's simple_tag reads the same two attributes)
    parser.add_argument('--num_adversaries', type=int, default=argparse.SUPPRESS,
                        help="simple_tag / simple_world_comm: agents 0 .. num_adversaries - 1 chase the others (3 / 4 where "
                             "not given)")
    parser.add_argument('--num_good_agents', type=int, default=argparse.SUPPRESS,
                        help="simple_tag / simple_world_comm: the agents that are chased (1 / 2 where not given); with --use_device_env "
                             "num_agents = num_adversaries + num_good_agents")
    return parser.parse_known_args(args)[0]


def main(args):
    all_args = parse_args(args, get_config())
    _launch.apply_algorithm_flags(all_args, ("rmappo", "mappo", "ippo", "happo", "hatrpo"))   # happo / hatrpo: separated runner
    assert (all_args.share_policy is True and all_args.scenario_name == 'simple_speaker_listener') is False, (
        "The simple_speaker_listener scenario can not use shared policy. Please check the config.py.")
    device = _launch.device_of(all_args)
    run_dir = _launch.new_run_dir(all_args, all_args.scenario_name)
    _launch.seed_everything(all_args)
    shared = all_args.share_policy and all_args.algorithm_name not in ("happo", "hatrpo")
    device_eval = bool(getattr(all_args, "use_device_eval", False))
    if device_eval and not (all_args.use_eval and all_args.use_device_env
                            and all_args.algorithm_name in ("rmappo", "mappo", "ippo")):
        raise NotImplementedError("--use_device_eval: with --use_eval and --use_device_env, rmappo / mappo / ippo only")
    if all_args.use_device_env:
        scenario = all_args.scenario_name
        separated = not shared and all_args.algorithm_name in ("rmappo", "mappo", "ippo")
        if not (scenario in DEVICE_ENVS and (separated if scenario in SEPARATED_DEVICE_ENVS else shared)):
            raise NotImplementedError(
                "--use_device_env: %s with the shared-policy runner, %s with the separated runner (rmappo / mappo / ippo) "
                "only" % (" / ".join(k for k in DEVICE_ENVS if k not in SEPARATED_DEVICE_ENVS),
                          " / ".join(SEPARATED_DEVICE_ENVS)))
        if scenario == "simple_push" and all_args.num_landmarks not in (1, 2):
            raise NotImplementedError("--use_device_env: simple_push colours landmark l on channel l + 1 of three, so "
                                      "--num_landmarks is 1 or 2 (the reference fails at 3), not %d"
                                      % all_args.num_landmarks)
        if scenario in KIND_DEFAULTS:
            adv, good = tag_counts(all_args)
            if adv < 1 or good < 1 or all_args.num_agents != adv + good:
                raise NotImplementedError("--use_device_env: %s needs num_agents = num_adversaries + "
                                          "num_good_agents with at least one of each, not %d = %d + %d"
                                          % (scenario, all_args.num_agents, adv, good))
        if scenario == "simple_world_comm" and all_args.num_landmarks < 1:
            raise NotImplementedError("--use_device_env: simple_world_comm needs at least one obstacle (--num_landmarks), "
                                      "not %d" % all_args.num_landmarks)
    envs = make_train_env(all_args, device=device if all_args.use_device_env else None)
    eval_envs = make_train_env(all_args, all_args.n_eval_rollout_threads, 50000,
                               device=device if device_eval else None) if all_args.use_eval else None
    if shared:
        from onpolicy.runner.shared.mpe_runner import MPERunner as Runner
    else:
        from onpolicy.runner.separated.mpe_runner import MPERunner as Runner
    return _launch.run(Runner, all_args, envs, eval_envs, all_args.num_agents, device, run_dir)


if __name__ == "__main__":
    main(sys.argv[1:])
