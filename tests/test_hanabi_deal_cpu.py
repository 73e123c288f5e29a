"""CPU side of the device Hanabi stepper (K16): its chance source against <random>, its argument checks, and the host
library after the rules moved into the shared header (csrc/hanabi_rules.h).

The deal is the one thing that must be library-identical to the reference engine: std::mt19937 +
std::discrete_distribution.  The device cannot call <random>, so hanabi_rules.h writes both out (Mt19937Strided,
pick_discrete); tests/hanabi_deal_check.cc -- a stand-alone program, built here under AddressSanitizer and UBSan --
draws from both side by side."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
from onpolicy import _native
from onpolicy.envs.hanabi import batch as hb

CHECK_SRC = os.path.join(ROOT, "tests", "hanabi_deal_check.cc")
FULL5 = (5, 5, 5, 0, 8, 3, 1, 0)          # Hanabi-Full, five players: the fields of hanabi_rules_t in order


def test_chance_source_equals_the_standard_library(tmp_path):
    """Seeds -3 .. 39 (negative seeds wrap modulo 2^32), 20,000 draws each over 1-25 weights built from counts 1-3 over
    their total, the generator's words 3 apart with guard words between them: every pick equals
    std::discrete_distribution's, single-weight draws consume nothing, both generators end at the same word, the
    guard words are intact, and every seed passes its 624 words at least three times."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "hanabi_deal_check")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", CHECK_SRC, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe, "20000"], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    got = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", run.stdout)}
    assert got["seeds"] == 43 and got["draws"] == 43 * 20000
    assert got["mismatches"] == 0 and got["desynced"] == 0 and got["trampled"] == 0
    assert got["min_refills"] >= 3 and got["single"] > 0


def _host(n, ctype=ctypes.c_float):
    """(keep-alive, address) of n elements, the address 16-byte aligned."""
    buf = (ctypes.c_uint8 * (n * ctypes.sizeof(ctype) + 16))()
    return buf, (ctypes.addressof(buf) + 15) & ~15


def test_device_stepper_validates_arguments_without_a_device():
    """Validation returns before anything is enqueued, so host buffers serve as pointers (no GPU here)."""
    lib = _native.lib()
    per_table = lib.mappo_hanabi_state_bytes(*FULL5)
    assert per_table >= 624 * 4 + 200 and per_table % 4 == 0
    dims = (ctypes.c_int32 * 5)()
    assert lib.mappo_hanabi_dims(*FULL5, ctypes.addressof(dims)) == 0
    ref = hb.HanabiBatch(dict(hb.rules_for("Hanabi-Full", 5)), [1])
    assert list(dims) == [5, ref.num_moves, ref.obs_len, ref.own_hand_len, 4]
    assert lib.mappo_hanabi_dims(*FULL5, None) == -1

    # rule sets outside the limits, and the start-player draw the device does not do
    bad_rules = [(6, 5, 5, 0, 8, 3, 1, 0), (5, 6, 2, 0, 8, 3, 1, 0), (5, 5, 6, 0, 8, 3, 1, 0), (5, 5, 1, 0, 8, 3, 1, 0),
                 (5, 5, 2, 6, 8, 3, 1, 0), (5, 5, 2, 0, -1, 3, 1, 0), (5, 5, 2, 0, 8, 0, 1, 0), (5, 5, 2, 0, 8, 3, 3, 0),
                 (1, 2, 5, 5, 8, 3, 1, 0), (5, 5, 5, 0, 8, 3, 1, 1), (5, 5, 5, 5, 100000, 3, 1, 0)]
    for rules in bad_rules:
        assert lib.mappo_hanabi_state_bytes(*rules) == -2, rules
        assert lib.mappo_hanabi_dims(*rules, ctypes.addressof(dims)) == -2, rules

    n = 2
    keep = {k: _host(16384) for k in ("state", "obs", "share", "avail", "rewards")}
    ints = {k: _host(64, ctypes.c_int32) for k in ("seeds", "actions", "scores", "to_move", "flags", "draws")}
    bytes_ = {k: _host(64, ctypes.c_uint8) for k in ("choose", "status")}
    p = {k: v[1] for d in (keep, ints, bytes_) for k, v in d.items()}

    def reset(**o):
        a = dict(dict(p, n=n, mode=0, rules=FULL5), **o)
        return lib.mappo_hanabi_reset(a["state"], a["choose"], a["obs"], a["share"], a["avail"], a["to_move"], a["flags"],
                                      a["n"], a["mode"], *a["rules"], None)

    def step(**o):
        a = dict(dict(p, n=n, mode=0, rules=FULL5), **o)
        return lib.mappo_hanabi_step(a["state"], a["actions"], a["rewards"], a["status"], a["scores"], a["obs"],
                                     a["share"], a["avail"], a["to_move"], a["flags"], a["n"], a["mode"], *a["rules"], None)

    def encode(**o):
        a = dict(dict(p, n=n, mode=0, rules=FULL5), **o)
        return lib.mappo_hanabi_encode(a["state"], a["choose"], a["obs"], a["share"], a["avail"], a["to_move"], a["n"],
                                       a["mode"], *a["rules"], None)

    for call, required in ((reset, ("state", "choose", "obs", "share", "avail", "flags")),
                           (step, ("state", "actions", "rewards", "status", "scores", "obs", "share", "avail", "flags")),
                           (encode, ("state", "obs", "share", "avail"))):
        for name in required:
            assert call(**{name: None}) == -1, (call.__name__, name)
        assert call(n=0) == -2 and call(n=-3) == -2 and call(n=(1 << 24) + 1) == -2
        assert call(mode=2) == -2 and call(mode=-1) == -2
        for rules in bad_rules:
            assert call(rules=rules) == -2, (call.__name__, rules)
        assert call(obs=p["obs"] + 4) == -5 and call(share=p["share"] + 8) == -5 and call(avail=p["avail"] + 4) == -5
        assert call(state=p["state"] + 2) == -5
    assert lib.mappo_hanabi_seed(None, p["seeds"], n, None) == -1
    assert lib.mappo_hanabi_seed(p["state"], None, n, None) == -1
    assert lib.mappo_hanabi_seed(p["state"], p["seeds"], 0, None) == -2
    assert lib.mappo_hanabi_draws(None, p["draws"], n, None) == -1
    assert lib.mappo_hanabi_draws(p["state"], None, n, None) == -1
    assert lib.mappo_hanabi_draws(p["state"], p["draws"], -1, None) == -2


def test_device_batch_refuses_a_cpu_device():
    """No quiet host stand-in behind the device classes."""
    from onpolicy.envs.hanabi.device import HanabiDeviceBatch
    with pytest.raises(NotImplementedError, match="GPU"):
        HanabiDeviceBatch(hb.rules_for("Hanabi-Small", 2), [1], device="cpu")


def test_host_library_still_exports_exactly_its_header():
    """The rules now come from a header that is full of inline functions and templates: none of them may leak into the
    library's C surface, and every function of include/hanabi_batch.h must still be there."""
    if shutil.which("nm") is None:
        pytest.skip("no nm")
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hanabi_batch.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(hanabi_batch_[a-z0-9_]+)\s*\(", src)))
    assert len(declared) == 13
    hb.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", hb.LIB_PATH], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    exported = [line.split()[-1] for line in out.stdout.splitlines() if line.strip()]
    c_surface = sorted(s for s in exported if not s.startswith("_"))       # C++ (mangled) and linker symbols aside
    assert c_surface == declared


def test_train_script_flag_is_opt_in_and_refuses_subproc_envs(monkeypatch, tmp_path):
    """--use_device_env: off unless given (the parsed namespace of a run without it is what it was), and not
    combinable with the one-env-per-thread layout; on a CPU device it is refused too."""
    import torch
    from onpolicy.config import get_config
    from onpolicy.scripts.train import _launch, train_hanabi_forward
    assert "use_device_env" not in vars(train_hanabi_forward.parse_args([], get_config()))
    assert train_hanabi_forward.parse_args(["--use_device_env"], get_config()).use_device_env is True
    monkeypatch.setattr(_launch, "device_of", lambda all_args: torch.device("cpu"))
    monkeypatch.setenv("MAPPO_RESULTS_DIR", str(tmp_path / "results"))
    common = ["--env_name", "Hanabi", "--hanabi_name", "Hanabi-Very-Small", "--num_agents", "2", "--algorithm_name",
              "mappo", "--n_rollout_threads", "2", "--use_wandb"]
    with pytest.raises(NotImplementedError, match="use_subproc_envs"):
        train_hanabi_forward.main(common + ["--use_device_env", "--use_subproc_envs"])
    with pytest.raises(NotImplementedError, match="GPU"):
        train_hanabi_forward.main(common + ["--use_device_env"])
