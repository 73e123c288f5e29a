"""What the compiler put between the matrix instructions of the six-term K9 kernels (tools/mfma_gaps.py; no GPU needed:
hipcc cross-compiles).  profiles/mfma_gaps.json holds the figures of the parent commit ("parent": the operand split
in one gap after every burst of 12 MFMAs) beside this tree's ("now": the split of the next step spread under the
MFMAs of the current one); here: the snapshot is what a fresh compile gives, and the two launches that read the critic's
384-wide rows expose fewer issue cycles than the parent's did."""
import importlib.util
import json
import os
import shutil

import pytest

from conftest import ROOT

SNAPSHOT = os.path.join(ROOT, "profiles", "mfma_gaps.json")
pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                                reason="hipcc not found")


def _tool():
    spec = importlib.util.spec_from_file_location("mfma_gaps", os.path.join(ROOT, "tools", "mfma_gaps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fresh():
    return _tool().collect()


def test_snapshot_matches_a_fresh_compile(fresh):
    snap = json.load(open(SNAPSHOT))
    assert set(snap["parent"]) == set(snap["now"]) == set(fresh)
    assert fresh == snap["now"], "the MFMA gaps changed -- rerun tools/mfma_gaps.py --write and review"


def test_critic_launches_expose_less_issue_than_the_parent(fresh):
    tool = _tool()
    snap = json.load(open(SNAPSHOT))
    for k in tool.CRITIC:
        now, parent = fresh[k], snap["parent"][k]
        print(k, "exposed cycles", parent["exposed_cycles"], "->", now["exposed_cycles"], "| empty gaps",
              parent["gaps_empty"], "->", now["gaps_empty"], "of", now["gaps"])
        assert now["mfma"] == parent["mfma"] and now["mfma_bf16"] == parent["mfma_bf16"]       # the same products
        assert now["exposed_cycles"] < parent["exposed_cycles"], (k, now, parent)


def test_first_layer_bursts_are_gone(fresh):
    """The critic forward's 24 first-layer steps are 288 of its MFMAs: in the parent's listing 310 of 367 gaps held no
    vector instruction at all (bursts of 12 MFMAs); with four split instructions placed in every gap of a step, fewer
    than half of the gaps can be empty (the hidden layer's and the head's float32 MFMAs still issue back to back)."""
    now = fresh["mlp_fwd4_kernel<1, 4, true>"]
    assert 2 * now["gaps_empty"] < now["gaps"], now


def test_cost_model_on_a_hand_made_listing():
    tool = _tool()
    body = ["v_mfma_f32_32x32x16_bf16 a[0:15], v[0:3], v[4:7], a[0:15]", "s_nop 7", "s_waitcnt lgkmcnt(0)",
            "v_mfma_f32_32x32x16_bf16 a[0:15], v[0:3], v[4:7], a[0:15]"] + ["v_sub_f32_e32 v1, v2, v3"] * 5 + [
            "v_exp_f32_e32 v1, v2", "ds_read_b128 v[0:3], v9", "v_pk_add_f32 v[0:1], v[2:3], v[4:5]",
            "v_mfma_f32_32x32x2_f32 a[0:15], v0, v1, a[0:15]", "v_add_f32_e32 v1, v2, v3"]
    assert tool.gaps_of(body) == [(2, 0, 9), (8, 8, 36)]
    m = tool.measure(body)
    assert (m["mfma"], m["mfma_bf16"], m["gaps"], m["gaps_empty"], m["exposed_cycles"], m["packed_f32"]) == (3, 2, 2, 1, 12, 1)
