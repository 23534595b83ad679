"""CPU: the BottleNeck inference fusion pass of the plan compiler (PlanBuilder.fuse_bottleneck, switched by LHN_INFER_FUSE_BNECK=1
or plan.set_infer_fuse_bneck) -- no GPU, no kernel launch -- and the non-degeneracy of the kernel cases of tests/bottleneck_cases.py
(float64 only).  A BottleNeck is: a stride-1 1x1 (128 -> Cm, Cm in {32, 64}) into a whole fresh buffer read by nothing but a stride-1
3x3 (Cm -> Cm), whose buffer is read by nothing but a 1x1 (Cm -> 128, slope 1), whose buffer is read by nothing but a plain
two-source sum with the first 1x1's input."""
import ctypes as C
import os
import re

import pytest
import torch
from torch import nn

import bottleneck_cases as bc
from litehandnet_amd import _lib, get_model, plan
from litehandnet_amd.config import litehandnet_cfg
from litehandnet_amd.plan import BNECK, CBAM, DWPW, EW, FINALIZE, KXK, MSRB, PW, PWDW, TABLE_FILL, PlanBuilder
from plan_digest import _deploy_without_gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("LHN_INFER_FUSE_BNECK", "LHN_INFER_FUSE_MSRB", "LHN_INFER_FUSE_DWPW", "LHN_INFER_FUSE")


@pytest.fixture(autouse=True)
def _switches_back(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    yield
    for f in (plan.set_infer_fuse, plan.set_infer_fuse_dwpw, plan.set_infer_fuse_msrb, plan.set_infer_fuse_bneck):
        f(None)


def _a_model(size=256, deployed=False, **kw):
    cfg = litehandnet_cfg("A", image_size=size, **kw)
    cfg.MODEL["ca_dropout"] = 0.0
    m = get_model(cfg)
    return _deploy_without_gpu(m) if deployed else m


def _builder(m, size, backward=False, n=2, **kw):
    tensors = list(m.state_dict(keep_vars=True).values())
    pb = PlanBuilder(n, {id(t): j for j, t in enumerate(tensors)}, image_hw=(size, size), with_backward=backward, p_drop=0.0, **kw)
    y = m.emit(pb, pb.image())
    if getattr(y, "buf", None) != -2:
        pb.set_output(y)
    return pb


OFF = dict(infer_fuse=False, infer_fuse_dwpw=False, infer_fuse_msrb=False)


def _ops(pb):
    cb, cf, cbw, nf, nb = pb.finalize()
    return [bytes(C.string_at(C.addressof(cf[i]), C.sizeof(cf[i]))) for i in range(nf)], cf, nf


@pytest.mark.parametrize("deployed", [False, True])
@pytest.mark.parametrize("size", [256, 224])
def test_variant_a_has_13_bottlenecks(size, deployed):
    pb = _builder(_a_model(size, deployed), size, infer_fuse_bneck=True, **OFF)
    _, cf, nf = _ops(pb)
    fused = [r for r in pb.recs if r["op"] == BNECK]
    assert len(fused) == 13 == pb.n_fused_bneck == sum(cf[i].kind == BNECK for i in range(nf))
    by_cm = sorted((r["mids"][0].C, r["x"].H) for r in fused)
    s = size // 4
    assert by_cm == sorted(6 * [(32, s // 8)] + 4 * [(32, s // 4)] + 2 * [(32, s // 2)] + [(64, s)])
    assert all(r["x"].C == 128 and r["out"].C == 128 and r["mids"][1].C == r["mids"][0].C and r["mids"][2].C == 128 for r in fused)
    assert not any(r["op"] == KXK and r["x"].C in (32, 64) and r["x"].C == r["out"].C and r["stride"] == 1 for r in pb.recs)
    # the op: x and two intermediates in in_buf, the third one's table in ws[0], the 3x3's scratch in ws[1], five parameter slots
    for i in range(nf):
        if cf[i].kind != BNECK:
            continue
        o = cf[i]
        assert min(o.in_buf) >= 0 and o.in_C[0] == 128 and o.in_C[1] == o.in_C[2] and o.in_C[1] in (32, 64) and o.out_C == 128
        assert o.ws[0] >= pb.table_base and o.ws[0] < pb.table_end and o.ws[1] >= 0
        assert o.p[0] >= 0 and o.p[2] >= 0 and o.p[3] >= 0 and (o.p[1] >= 0) == deployed == (o.p[4] >= 0)
        assert o.f[0] == pytest.approx(0.01)


def test_reduction_2_is_all_cm_64():
    pb = _builder(_a_model(256, reduction=2), 256, infer_fuse_bneck=True, **OFF)
    pb.finalize()
    fused = [r for r in pb.recs if r["op"] == BNECK]
    assert len(fused) == 13 and all(r["mids"][0].C == 64 for r in fused)


def test_silu_blocks_are_left_alone():
    pb = _builder(_a_model(256, activation="silu"), 256, infer_fuse_bneck=True, **OFF)
    pb.finalize()
    assert pb.n_fused_bneck == 0 and not any(r["op"] == BNECK for r in pb.recs)


def test_training_plans_are_never_rewritten():
    m = _a_model(64)
    want = _ops(_builder(m, 64, True, infer_fuse_bneck=False))[0]
    got = _builder(m, 64, True, infer_fuse_bneck=True)
    assert _ops(got)[0] == want and got.n_fused_bneck == 0 and not any(r["op"] == BNECK for r in got.recs)


def test_switch_off_changes_nothing():
    m = _a_model(256)
    want = _ops(_builder(m, 256))[0]                                 # built without the argument
    new = _builder(m, 256, infer_fuse_bneck=False)
    assert _ops(new)[0] == want and new.n_fused_bneck == 0 and not any(r["op"] == BNECK for r in new.recs)
    on = _builder(m, 256, infer_fuse_bneck=True)
    assert _ops(on)[0] != want


def test_set_none_falls_back_to_the_environment(monkeypatch):
    m = _a_model(64)
    assert not plan.infer_fuse_bneck_enabled()
    plan.set_infer_fuse_bneck(True)
    assert plan.infer_fuse_bneck_enabled() and _builder(m, 64, infer_fuse_bneck=None).infer_fuse_bneck
    plan.set_infer_fuse_bneck(False)
    monkeypatch.setenv("LHN_INFER_FUSE_BNECK", "1")
    assert not plan.infer_fuse_bneck_enabled()
    plan.set_infer_fuse_bneck(None)
    assert plan.infer_fuse_bneck_enabled() and not plan.infer_fuse_enabled() and not plan.infer_fuse_dwpw_enabled() and \
        not plan.infer_fuse_msrb_enabled()
    pb = _builder(m, 64, infer_fuse_bneck=None)
    pb.finalize()
    assert pb.infer_fuse_bneck and pb.n_fused_bneck == 13
    assert not _builder(m, 64).infer_fuse_bneck                     # the argument's default is off, whatever the environment says
    monkeypatch.delenv("LHN_INFER_FUSE_BNECK")
    assert not plan.infer_fuse_bneck_enabled()


@pytest.mark.parametrize("variant", ["A", "B"])
def test_all_four_switches_on(variant):
    cfg = litehandnet_cfg(variant, image_size=256)
    cfg.MODEL["ca_dropout"] = 0.0
    m = get_model(cfg)
    # the BottleNeck pass finds alone what it finds with the others on, and the other three find with it what they find without
    # it.  (Among themselves the older passes are not independent on variant A: fuse_dw_pw runs first and takes the depthwise
    # convolution of a 1x1 -> depthwise -> 1x1 chain, so fuse_pw_dw's count with it on differs from its count alone.)
    alone = _builder(m, 256, infer_fuse_bneck=True, **OFF)
    alone.finalize()
    three = _builder(m, 256, infer_fuse=True, infer_fuse_dwpw=True, infer_fuse_msrb=True, infer_fuse_bneck=False)
    three.finalize()
    on = _builder(m, 256, infer_fuse=True, infer_fuse_dwpw=True, infer_fuse_msrb=True, infer_fuse_bneck=True)
    on.finalize()
    assert (on.n_fused, on.n_fused_dwpw, on.n_fused_msrb) == (three.n_fused, three.n_fused_dwpw, three.n_fused_msrb)
    assert on.n_fused_bneck == alone.n_fused_bneck and three.n_fused_bneck == 0
    for k in ("infer_fuse", "infer_fuse_dwpw", "infer_fuse_msrb"):   # each of them alone, with and without the new pass
        a = _builder(m, 256, **{**OFF, "infer_fuse_bneck": False, k: True})
        b = _builder(m, 256, **{**OFF, "infer_fuse_bneck": True, k: True})
        a.finalize(), b.finalize()
        assert (a.n_fused, a.n_fused_dwpw, a.n_fused_msrb) == (b.n_fused, b.n_fused_dwpw, b.n_fused_msrb) and b.n_fused_bneck == alone.n_fused_bneck
    for kind in (PWDW, DWPW, MSRB):
        assert [(id(r["conv"]), id(r["conv2"])) for r in on.recs if r["op"] == kind] == \
               [(id(r["conv"]), id(r["conv2"])) for r in three.recs if r["op"] == kind]
    assert on.n_fused_bneck == (13 if variant == "A" else 0)
    claimed = [id(c) for r in on.recs if r["op"] in (MSRB, PWDW, DWPW) for c in (r["conv"], r["conv2"])]
    claimed += [id(c) for r in on.recs if r["op"] == BNECK for c in r["convs"]]
    assert len(claimed) == len(set(claimed))                         # no convolution is claimed twice


@pytest.mark.parametrize("deployed", [False, True])
def test_intermediates_keep_tables_and_lose_data(deployed):
    m = _a_model(64, deployed)
    off = _builder(m, 64, infer_fuse_bneck=False, **OFF)
    off.finalize()
    on = _builder(m, 64, infer_fuse_bneck=True, **OFF)
    _, cf, nf = _ops(on)
    fused = [r for r in on.recs if r["op"] == BNECK]
    assert {r["x"].H for r in fused} == {16, 8, 4, 2}
    assert not any(r["op"] == FINALIZE for r in off.recs)
    for r in fused:
        j = next(i for i, q in enumerate(on.recs) if q is r)
        for k, t in enumerate(r["mids"]):
            b = on.bufs[t.buf]
            assert b.fused and b.off["data"] == -1 and b.off["table"] >= 0
            fills = [i for i, q in enumerate(on.recs) if q["op"] in (FINALIZE, TABLE_FILL) and q["out"].buf == t.buf]
            # eval: one FINALIZE per intermediate; deployed: the 3x3's bias (the 1x1 biases ride in the launch, their slope is 1)
            assert len(fills) == (1 if not deployed else (1 if k == 1 else 0)), (k, fills)
            assert all(i < j for i in fills)
            assert all(on.recs[i]["op"] == (TABLE_FILL if deployed else FINALIZE) for i in fills)
            # nothing else touches the intermediate
            assert not any(v.buf == t.buf for q in on.recs if q is not r and q["op"] not in (FINALIZE, TABLE_FILL)
                           for val in q.values() for v in plan._refs_in(val))
        assert (r["b1"] is not None) == deployed == (r["b3"] is not None)
    # the workspace shrinks by the intermediates' data
    assert on.act_bytes < off.act_bytes
    # three convolutions and the sum leave per block; eval adds the three FINALIZE records
    n_conv = lambda pb: sum(r["op"] in (PW, KXK) for r in pb.recs)
    n_ew = lambda pb: sum(r["op"] == EW and not r.get("lazy") for r in pb.recs)
    assert n_conv(off) - n_conv(on) == 39 and n_ew(off) - n_ew(on) == 13


def test_symbol_is_declared_listed_and_exported():
    with open(os.path.join(ROOT, "include", "lhn.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+lhn_bottleneck_fwd\s*\(", header)
    so = C.CDLL(_lib.LIB_PATH)
    assert "lhn_bottleneck_fwd" in _lib.SYMBOLS and hasattr(so, "lhn_bottleneck_fwd")
    L = _lib.lib()
    assert len(L.lhn_bottleneck_fwd.argtypes) == 14 and L.lhn_version() == 3
    assert BNECK == CBAM + 1


# ---------------------------------------------------------------- the kernel cases are not degenerate (float64, reference alone)
SMALL = [k for k, c in bc.CASES.items() if c["n"] <= 5]


def test_case_table_covers_what_it_must():
    for cm in (32, 64):
        sizes = {(c["h"], c["w"]) for c in bc.CASES.values() if c["cm"] == cm}
        assert {(1, 5), (2, 3), (4, 4), (7, 7), (8, 8), (14, 14), (16, 16), (28, 28), (32, 32), (9, 70), (24, 40), (12, 70)} <= sizes
        assert {c["out_slope"] for c in bc.CASES.values() if c["cm"] == cm} >= {0.0, 0.01, 1.0}
        assert {c["slopes"][:2] for c in bc.CASES.values() if c["cm"] == cm} >= {(0.0, 0.0), (1.0, 1.0)}
        for j in range(3):
            assert any(not c["tabs"][j] and all(c["tabs"][i] for i in range(3) if i != j) for c in bc.CASES.values() if c["cm"] == cm)
        for j in range(2):
            assert any(not c["biases"][j] and c["biases"][1 - j] for c in bc.CASES.values() if c["cm"] == cm)
    assert (56, 56) in {(c["h"], c["w"]) for c in bc.CASES.values() if c["cm"] == 64}
    for name, c in bc.CASES.items():
        assert 2 <= c["n"] <= 5 or name.startswith("multi_item") or (c["n"] == 1 and c["w"] == 70), name
        assert c["x"][1] + 128 <= c["x"][0] and c["y"][1] + 128 <= c["y"][0], name


@pytest.mark.parametrize("name", SMALL)
def test_case_is_not_degenerate(name):
    """At least 10 % of the pre-activation elements of t1, t2 and of the final sum are negative and at least 10 % positive: every
    slope matters.  Shift-far cases: the reference differs at border pixels from the wrong-padding variant by > 100 floors."""
    c = bc.CASES[name]
    g = bc.inputs(name)
    y, p1, p2, s = bc.reference(name, g, parts=True)
    assert y.shape == (c["n"], c["h"], c["w"], 128) and bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0.1
    for what, p in (("t1", p1), ("t2", p2), ("sum", s)):
        neg, pos = float((p < 0).double().mean()), float((p > 0).double().mean())
        assert neg >= 0.10 and pos >= 0.10, (name, what, neg, pos)
    if c["shift_far"]:
        wrong = bc.reference(name, g, wrong_padding=True)
        b = bc.border(c["h"], c["w"])
        peak = float(y.abs().max())
        d_border = float((wrong - y)[:, b].abs().max()) / peak
        assert d_border > 100 * bc.FLOOR, (name, d_border)
        if bool((~b).any()) and c["h"] > 2 and c["w"] > 2:           # and only there
            assert float((wrong - y)[:, ~b].abs().max()) < 1e-9 * peak
    if c["const"]:
        assert float((y - bc.const_answer(name)).abs().max()) < 1e-7      # (1 / (9 Cm) is rounded to float32 in the inputs)
