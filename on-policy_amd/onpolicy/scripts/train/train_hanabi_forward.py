#!/usr/bin/env python
"""Train script for Hanabi (turn-based runner) -- flags and flow of the reference's
onpolicy/scripts/train/train_hanabi_forward.py (parse_args :61-69, env factories :16-58, runner :158-162).
The env is the in-tree batched stepper (``onpolicy.envs.hanabi``): all rollout threads advance in one native
call (``HanabiBatchVecEnv``).  ``--use_subproc_envs`` builds the reference's layout instead -- one ``HanabiEnv``
per thread behind ``ChooseSubprocVecEnv`` / ``ChooseDummyVecEnv``; both give identical games for the same seeds.
``--use_device_env`` keeps the TRAINING tables in device memory instead (``HanabiDeviceVecEnv``: HIP stepper and encoder,
same games again); where the evaluation plays is a flag of its own:
``--use_device_eval`` (with ``--use_eval``; opt-in, independent of ``--use_device_env``) keeps the EVAL tables in device memory
and plays an evaluation without the host: the deterministic action (K14 mode), the env step (K16) and the bookkeeping between
them (K18: runner/shared/hanabi_eval.py) are launches only, a move is replayed from a captured graph, and the host reads one
block of counters every few rounds.  Without it evaluation runs on the host stepper, move by move.
``--use_device_turns`` (with ``--use_device_env``; opt-in) also takes the turn bookkeeping off the host: who moves and which
games restart are read off the tables' flags words on the device (K17), the policy runs on all N rows, and a player's move is
replayed from a captured graph -- a buffer step copies nothing to the host.  Same game, same policy, but NOT the default
route's trajectories: the sampler's noise tensor is [N, moves] instead of [movers, moves], so the same generator state gives
different draws as soon as one table sits a move out (another sample of the same distribution; see
runner/shared/hanabi_runner_forward.py).  A recurrent policy (``--use_recurrent_policy``, ``--use_naive_recurrent_policy``)
stays on the default device route under ``--use_device_turns`` alone; ``--use_device_turns_rnn`` (with it; opt-in) puts it on
the host-free route as well: the two launches of K17 then also keep the actor's and the critic's RNN state per (table, player).

    python -m onpolicy.scripts.train.train_hanabi_forward --env_name Hanabi --hanabi_name Hanabi-Full --num_agents 2 ...
"""
import argparse
import sys

from onpolicy.config import get_config
from onpolicy.envs.env_wrappers import ChooseDummyVecEnv, ChooseSubprocVecEnv
from onpolicy.scripts.train import _launch


def make_env(all_args, n_threads, seed_of_rank, device=None):
    """``device``: build the tables in that device's memory (the training envs under ``--use_device_env``, the eval envs
    under ``--use_device_eval``)."""
    if all_args.env_name != "Hanabi":
        raise NotImplementedError("Can not support the " + all_args.env_name + " environment.")
    assert 1 < all_args.num_agents < 6, "num_agents can be only between 2-5."
    if device is not None:
        from onpolicy.envs.hanabi.device import HanabiDeviceVecEnv
        return HanabiDeviceVecEnv(all_args, [seed_of_rank(rank) for rank in range(n_threads)], device)
    if not all_args.use_subproc_envs:
        from onpolicy.envs.hanabi.batch import HanabiBatchVecEnv
        # the runner copies every row it keeps, so the stepper's own arrays are handed out as they are
        return HanabiBatchVecEnv(all_args, [seed_of_rank(rank) for rank in range(n_threads)], copy=False)

    def get_env_fn(rank):
        def init_env():
            if all_args.env_name != "Hanabi":
                raise NotImplementedError("Can not support the " + all_args.env_name + " environment.")
            assert 1 < all_args.num_agents < 6, "num_agents can be only between 2-5."
            from onpolicy.envs.hanabi.Hanabi_Env import HanabiEnv
            env = HanabiEnv(all_args, seed_of_rank(rank))
            env.seed(seed_of_rank(rank))
            return env
        return init_env
    if n_threads == 1:
        return ChooseDummyVecEnv([get_env_fn(0)])
    return ChooseSubprocVecEnv([get_env_fn(i) for i in range(n_threads)])


def parse_args(args, parser):
    parser.add_argument('--hanabi_name', type=str, default='Hanabi-Very-Small', help="Which env to run on")
    parser.add_argument('--num_agents', type=int, default=2, help="number of players")
    parser.add_argument('--use_subproc_envs', action='store_true', default=False,
                        help="one HanabiEnv per rollout thread behind the Choose* VecEnv wrappers (reference layout) "
                             "instead of the batched stepper")
    # opt-in and absent from the namespace unless given (main() reads it as False then): a run without it parses
    # exactly as before
    parser.add_argument('--use_device_env', action='store_true', default=argparse.SUPPRESS,
                        help="keep the training tables on the GPU (HIP stepper and encoder); the eval tables follow "
                             "--use_device_eval")
    parser.add_argument('--use_device_turns', action='store_true', default=argparse.SUPPRESS,
                        help="with --use_device_env: turn bookkeeping on the GPU too (no device -> host copy per move, "
                             "moves replayed from captured graphs); samples other trajectories than the default route")
    parser.add_argument('--use_device_turns_rnn', action='store_true', default=argparse.SUPPRESS,
                        help="with --use_device_turns: a recurrent policy takes the host-free route too (its RNN states are "
                             "kept by the turn kernels); changes nothing for a feed-forward policy")
    parser.add_argument('--use_device_eval', action='store_true', default=argparse.SUPPRESS,
                        help="with --use_eval: keep the EVAL tables on the GPU and play the evaluation without the host "
                             "(K18, captured moves); independent of --use_device_env")
    return parser.parse_known_args(args)[0]


def check_device_eval(all_args, device=None):
    """-> whether ``--use_device_eval`` was given; refuses the combinations it cannot serve (``device``: once it is known)."""
    if not getattr(all_args, "use_device_eval", False):
        return False
    if not all_args.use_eval:
        raise NotImplementedError("--use_device_eval needs --use_eval (it only changes how the evaluation is played)")
    if all_args.use_subproc_envs:
        raise NotImplementedError("--use_device_eval and --use_subproc_envs are two different env layouts: pick one")
    if device is not None and device.type != "cuda":
        raise NotImplementedError("--use_device_eval needs a GPU device (the eval tables live in its memory)")
    return True


def main(args):
    all_args = _launch.apply_algorithm_flags(parse_args(args, get_config()), ("rmappo", "mappo", "ippo"))
    all_args.use_device_env = bool(getattr(all_args, "use_device_env", False))
    if getattr(all_args, "use_device_turns", False) and not all_args.use_device_env:
        raise NotImplementedError("--use_device_turns needs --use_device_env (it drives the tables in device memory)")
    if getattr(all_args, "use_device_turns_rnn", False) and not getattr(all_args, "use_device_turns", False):
        raise NotImplementedError("--use_device_turns_rnn needs --use_device_turns (it lets a recurrent policy take that route)")
    check_device_eval(all_args)
    device = _launch.device_of(all_args)
    device_eval = check_device_eval(all_args, device)
    if all_args.use_device_env and all_args.use_subproc_envs:
        raise NotImplementedError("--use_device_env and --use_subproc_envs are two different env layouts: pick one")
    if all_args.use_device_env and device.type != "cuda":
        raise NotImplementedError("--use_device_env needs a GPU device (the tables live in its memory)")
    run_dir = _launch.new_run_dir(all_args, all_args.hanabi_name)
    _launch.seed_everything(all_args)
    envs = make_env(all_args, all_args.n_rollout_threads, lambda rank: all_args.seed + (getattr(all_args, "rollout_thread_offset", 0) + rank) * 1000,
                    device=device if all_args.use_device_env else None)
    eval_envs = make_env(all_args, all_args.n_eval_rollout_threads,
                         lambda rank: all_args.seed * 50000 + rank * 10000,
                         device=device if device_eval else None) if all_args.use_eval else None
    if not all_args.share_policy:
        raise NotImplementedError("the separated Hanabi runner is outside this implementation")
    from onpolicy.runner.shared.hanabi_runner_forward import HanabiRunner as Runner
    return _launch.run(Runner, all_args, envs, eval_envs, all_args.num_agents, device, run_dir)


if __name__ == "__main__":
    main(sys.argv[1:])
