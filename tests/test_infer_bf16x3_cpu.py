"""CPU: the split-bf16 pass of the plan compiler (PlanBuilder.mark_bf16x3, switched by LHN_INFER_BF16X3=1 or plan.set_infer_bf16x3)
-- no GPU, no kernel launch.  The pass marks the dense 3x3 records plan.bf16x3_eligible accepts, in plans without a backward; a marked
record lowers to the same KXK op with i[1] = 1 and nothing else in the op arrays moves."""
import ctypes as C
import json
import os
import re

import pytest

import plan_digest
from litehandnet_amd import _lib, get_model, plan
from litehandnet_amd.config import litehandnet_cfg
from litehandnet_amd.plan import BNECK, KXK, PlanBuilder

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SWITCHES = ("LHN_INFER_BF16X3", "LHN_INFER_FUSE_BNECK", "LHN_INFER_FUSE_MSRB", "LHN_INFER_FUSE_DWPW", "LHN_INFER_FUSE")
SETTERS = (plan.set_infer_bf16x3, plan.set_infer_fuse_bneck, plan.set_infer_fuse_msrb, plan.set_infer_fuse_dwpw, plan.set_infer_fuse)
FOUR = dict(infer_fuse=True, infer_fuse_dwpw=True, infer_fuse_msrb=True, infer_fuse_bneck=True)
# dense 3x3 records at N = 2, 256 x 256: (marked, all).  Stride 1 with 32 / 64 / 128 channels: A 22, M 22, H 31; the 32 -> 32 class
# (12 in A, 13 in M) was taken out of the eligibility function by measurement (plan.BF16X3_LEFT_OUT)
COUNTS = {"A": (10, 26), "M": (9, 26), "H": (31, 31), "B": (0, 0), "L": (0, 0)}
SUPPORTED = {"A": 22, "M": 22, "H": 31, "B": 0, "L": 0}

with open(os.path.join(HERE, "plan_digests.json")) as _f:
    PINNED = json.load(_f)["configs"]


@pytest.fixture(autouse=True)
def _switches_back(monkeypatch):
    for name in SWITCHES + plan_digest.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    yield
    for f in SETTERS:
        f(None)


_MODELS = {}


def _model(variant):
    if variant not in _MODELS:
        cfg = litehandnet_cfg(variant, image_size=256)
        cfg.MODEL["ca_dropout"] = 0.0
        _MODELS[variant] = get_model(cfg)
    return _MODELS[variant]


def _builder(variant, backward=False, **kw):
    m = _model(variant)
    tensors = list(m.state_dict(keep_vars=True).values())
    pb = PlanBuilder(2, {id(t): j for j, t in enumerate(tensors)}, image_hw=(256, 256), with_backward=backward, p_drop=0.0, **kw)
    y = m.emit(pb, pb.image())
    if getattr(y, "buf", None) != -2:
        pb.set_output(y)
    return pb


def _ops(pb):
    cb, cf, cbw, nf, nb = pb.finalize()
    raw = lambda arr, n: [bytes(C.string_at(C.addressof(arr[i]), C.sizeof(arr[i]))) for i in range(n)]  # noqa: E731
    return cf, nf, raw(cf, nf), (raw(cbw, nb) if nb else []), bytes(C.string_at(C.addressof(cb), C.sizeof(cb)))


def _eligible(r):
    x, y = r["x"], r["out"]
    return plan.bf16x3_eligible(x.C, y.C, r["stride"], x.buf == y.buf and x.coff < y.coff + y.C and y.coff < x.coff + x.C)


@pytest.mark.parametrize("variant", ["A", "M", "H"])
def test_switch_off_is_the_pinned_plan(variant):
    pb = _builder(variant, infer_bf16x3=False)
    assert plan_digest.digest(pb) == PINNED[f"{variant}_fwd"]
    assert pb.n_bf16x3 == 0 and not any(r.get("bf16x3") for r in pb.recs)
    assert plan_digest.digest(_builder(variant)) == PINNED[f"{variant}_fwd"]          # the argument's default is off


@pytest.mark.parametrize("variant", ["A", "M", "H", "B", "L"])
def test_switch_on_marks_exactly_the_eligible_records(variant):
    off = _builder(variant, infer_bf16x3=False)
    _, nf0, ops0, _, bufs0 = _ops(off)
    on = _builder(variant, infer_bf16x3=True)
    cf, nf, ops1, _, bufs1 = _ops(on)
    assert nf == nf0 and bufs1 == bufs0 and (on.total_bytes, on.act_bytes) == (off.total_bytes, off.act_bytes)
    kxk = [r for r in on.recs if r["op"] == KXK]
    want = [r for r in kxk if r["stride"] == 1 and _eligible(r)]
    assert (len(want), len(kxk)) == COUNTS[variant] and on.n_bf16x3 == len(want)
    assert [id(r) for r in kxk if r.get("bf16x3")] == [id(r) for r in want]
    left = [r for r in kxk if not r.get("bf16x3")]
    assert all(r["stride"] == 2 or r["out"].C not in plan.BF16X3_CHANNELS or r["x"].C not in plan.BF16X3_CHANNELS or
               (r["x"].C, r["out"].C) in plan.BF16X3_LEFT_OUT for r in left)
    assert len(kxk) - sum(r["stride"] == 2 or r["out"].C not in plan.BF16X3_CHANNELS or r["x"].C not in plan.BF16X3_CHANNELS for r in kxk) == SUPPORTED[variant]
    # the op arrays: the marked KXK ops carry i[1] = 1 and a scratch; every other byte is the switch-off plan's
    marked = [i for i in range(nf) if cf[i].kind == KXK and cf[i].i[1] == 1]
    assert len(marked) == len(want) and all(cf[i].i[0] == 1 and cf[i].ws[3] >= 0 for i in marked)
    assert [(cf[i].in_C[0], cf[i].out_C) for i in marked] == [(r["x"].C, r["out"].C) for r in want]
    assert not any(cf[i].i[1] for i in range(nf) if cf[i].kind == KXK and i not in marked)
    for i in marked:
        cf[i].i[1] = 0
    again = [bytes(C.string_at(C.addressof(cf[i]), C.sizeof(cf[i]))) for i in range(nf)]
    assert again == ops0
    assert [i for i in range(nf) if ops1[i] != ops0[i]] == marked


@pytest.mark.parametrize("variant", ["A", "H"])
def test_plans_with_a_backward_are_never_marked(variant):
    off = _builder(variant, True, infer_bf16x3=False)
    _, _, f0, b0, _ = _ops(off)
    on = _builder(variant, True, infer_bf16x3=True)
    cf, nf, f1, b1, _ = _ops(on)
    assert (f1, b1) == (f0, b0) and on.n_bf16x3 == 0 and not any(r.get("bf16x3") for r in on.recs)
    assert not any(cf[i].i[1] for i in range(nf) if cf[i].kind == KXK)
    assert plan_digest.digest(_builder(variant, True, infer_bf16x3=True)) == PINNED[f"{variant}_bwd"]


@pytest.mark.parametrize("variant", ["A", "M", "H"])
def test_composes_with_the_four_fusion_switches(variant):
    """The fusion passes find with it what they find without it; a BNECK record keeps its fp32 inner 3x3 and this pass takes the 3x3
    records that are left."""
    four = _builder(variant, infer_bf16x3=False, **FOUR)
    _, nf0, ops0, _, _ = _ops(four)
    five = _builder(variant, infer_bf16x3=True, **FOUR)
    cf, nf, ops1, _, _ = _ops(five)
    assert (five.n_fused, five.n_fused_dwpw, five.n_fused_msrb, five.n_fused_bneck) == (four.n_fused, four.n_fused_dwpw, four.n_fused_msrb, four.n_fused_bneck)
    left = [r for r in five.recs if r["op"] == KXK and r["stride"] == 1 and _eligible(r)]
    if variant == "A":      # the 13 inner 3x3 are twelve 32 -> 32 (left out anyway) and one 64 -> 64
        assert five.n_fused_bneck == 13 and sum(r["op"] == BNECK for r in five.recs) == 13
        assert five.n_bf16x3 == len(left) == COUNTS["A"][0] - 1
    else:
        assert five.n_fused_bneck == 0 and five.n_bf16x3 == len(left) == COUNTS[variant][0]
    inner = {id(r["convs"][1]) for r in five.recs if r["op"] == BNECK}
    assert not inner & {id(r["conv"]) for r in left}
    marked = [i for i in range(nf) if cf[i].kind == KXK and cf[i].i[1] == 1]
    assert nf == nf0 and len(marked) == len(left) and [i for i in range(nf) if ops1[i] != ops0[i]] == marked


def test_set_none_falls_back_to_the_environment(monkeypatch):
    assert not plan.infer_bf16x3_enabled()
    plan.set_infer_bf16x3(True)
    assert plan.infer_bf16x3_enabled() and _builder("A", infer_bf16x3=None).infer_bf16x3
    plan.set_infer_bf16x3(False)
    monkeypatch.setenv("LHN_INFER_BF16X3", "1")
    assert not plan.infer_bf16x3_enabled()
    plan.set_infer_bf16x3(None)
    assert plan.infer_bf16x3_enabled() and not plan.infer_fuse_enabled() and not plan.infer_fuse_bneck_enabled()
    pb = _builder("A", infer_bf16x3=None)
    pb.finalize()
    assert pb.infer_bf16x3 and pb.n_bf16x3 == 10
    assert not _builder("A").infer_bf16x3                             # the argument's default is off, whatever the environment says
    monkeypatch.delenv("LHN_INFER_BF16X3")
    assert not plan.infer_bf16x3_enabled()


def test_eligibility_rule():
    for ci in (16, 32, 48, 64, 96, 128, 256):
        for co in (16, 32, 48, 64, 96, 128, 256):
            ok = ci in (32, 64, 128) and co in (32, 64, 128) and (ci, co) != (32, 32)
            assert plan.bf16x3_eligible(ci, co, 1) == ok
            assert not plan.bf16x3_eligible(ci, co, 2) and not plan.bf16x3_eligible(ci, co, 1, overlap=True)


def test_symbol_is_declared_listed_and_exported():
    with open(os.path.join(ROOT, "include", "lhn.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+lhn_conv_kxk_fwd_bf16x3\s*\(", header)
    so = C.CDLL(_lib.LIB_PATH)
    assert "lhn_conv_kxk_fwd_bf16x3" in _lib.SYMBOLS and hasattr(so, "lhn_conv_kxk_fwd_bf16x3")
    L = _lib.lib()
    assert len(L.lhn_conv_kxk_fwd_bf16x3.argtypes) == 6 and L.lhn_version() == 3
