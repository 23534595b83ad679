"""CPU: the op lists of the plan compiler are byte-identical to the ones pinned in tests/plan_digests.json (written by
tests/plan_digest.py at the commit in that file's "generated_at" field) -- for every model variant, with and without a
backward, and with every plan switch off.  The file is not regenerated when a hash differs: dump the configuration in both
trees and diff the text."""
import json
import os

import pytest

from litehandnet_amd import plan

import plan_digest

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "plan_digests.json")) as _f:
    PINNED = json.load(_f)["configs"]


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
