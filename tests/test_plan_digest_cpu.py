"""CPU: the op lists of the plan compiler are byte-identical to the ones pinned in tests/plan_digests.json (written by
tests/plan_digest.py at the commit in that file's "generated_at" field) -- for every model variant, with and without a
backward, and with every plan switch off -- and, for plans without a backward under the six inference switches, to the ones
pinned in tests/plan_digests_infer.json (eval and deployed form, each switch alone and all six together).  Neither file is
regenerated when a hash differs: dump the configuration in both trees and diff the text."""
import json
import os

import pytest

from litehandnet_amd import plan

import plan_digest

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "plan_digests.json")) as _f:
    PINNED = json.load(_f)["configs"]
with open(os.path.join(HERE, "plan_digests_infer.json")) as _f:
    PINNED_INFER = json.load(_f)["configs"]


@pytest.fixture(autouse=True)
def _switch_back():
    yield
    plan.set_infer_fuse(None)


def test_every_configuration_is_pinned():
    assert sorted(PINNED) == sorted(plan_digest.CONFIGS) and len(PINNED) == 29


@pytest.mark.parametrize("name", list(plan_digest.CONFIGS))
def test_op_lists_are_unchanged(name, monkeypatch):
    for s in plan_digest.SWITCHES + ("LHN_INFER_FUSE",):
        monkeypatch.delenv(s, raising=False)
    for s in plan_digest.CONFIGS[name]["off"]:
        monkeypatch.setenv(s, "0")
    got = plan_digest.digest(plan_digest.build(name))
    assert got == PINNED[name], (f"{name}: the plan differs from the pinned one; compare the output of "
                                 f"`python tests/plan_digest.py --dump '{name}'` in this tree and at the pinned commit")


def test_every_inference_configuration_is_pinned():
    # A, B, M x 2 forms x (6 switches alone + all six) + A, B at 224 x 2 forms + H, L and one hourglass_ablation
    assert sorted(PINNED_INFER) == sorted(plan_digest.INFER_CONFIGS) and len(PINNED_INFER) == 3 * 2 * 7 + 2 * 2 + 3 == 49


@pytest.mark.parametrize("deployed", [False, True])
@pytest.mark.parametrize("kw", plan_digest.INFER_KW)
def test_every_inference_pass_fires_in_a_pinned_configuration(kw, deployed):
    """A table in which a pass never rewrites anything pins nothing about that pass: every one of the six has a non-zero count
    in at least one pinned configuration of each form, and never where its switch is off."""
    counter = plan_digest.INFER_COUNTER_OF[kw]
    fired = [name for name, c in plan_digest.INFER_CONFIGS.items()
             if c["deployed"] == deployed and kw in c["on"] and PINNED_INFER[name]["counters"][counter] > 0]
    assert fired, f"{counter} is zero in every pinned {'deployed' if deployed else 'eval'} configuration"
    assert not [name for name, c in plan_digest.INFER_CONFIGS.items() if kw not in c["on"] and PINNED_INFER[name]["counters"][counter]]


@pytest.mark.parametrize("name", list(plan_digest.INFER_CONFIGS))
def test_inference_op_lists_are_unchanged(name, monkeypatch):
    for s in plan_digest.SWITCHES + plan_digest.INFER_ENV:
        monkeypatch.delenv(s, raising=False)
    got = plan_digest.infer_digest(plan_digest.build(name))
    assert got == PINNED_INFER[name], (f"{name}: the plan differs from the pinned one; compare the output of "
                                       f"`python tests/plan_digest.py --dump '{name}'` in this tree and at the pinned commit")
