"""CPU: the BottleNeck inference fusion pass (PlanBuilder.fuse_bottleneck) on variant A at channels=256 -- the width of the
reference's litehandnet `_w256` / `h4_ca_none` configs -- and the non-degeneracy of the kernel cases of tests/bottleneck256_cases.py
(float64 only).  No GPU, no kernel launch.  lhn_bottleneck_fwd takes 256 -> 64 -> 256 and 256 -> 128 -> 256, and both classes are in
PlanBuilder.FUSE_BNECK_CHANNELS (profiles/infer_fuse_bneck256.md has the measurement each class was kept on), so all thirteen
BottleNecks of the model are rewritten at either reduction.  The plan is all that exists of variant A at this width: on the GPU its
256 -> 256 dense 3x3 (BasicBlock) has no kernel, so tests/test_infer_fuse_bneck256_gpu.py runs the thirteen blocks without it."""
import ctypes as C

import pytest
import torch

import bottleneck256_cases as bc
from litehandnet_amd import get_model, plan
from litehandnet_amd.config import litehandnet_cfg
from litehandnet_amd.plan import BNECK, EW, KXK, PW, PlanBuilder
from plan_digest import _deploy_without_gpu

SWITCHES = ("LHN_INFER_FUSE_BNECK", "LHN_INFER_FUSE_MSRB", "LHN_INFER_FUSE_DWPW", "LHN_INFER_FUSE", "LHN_INFER_BF16X3", "LHN_INFER_FUSE_STEM")
OFF = dict(infer_fuse=False, infer_fuse_dwpw=False, infer_fuse_msrb=False)


@pytest.fixture(autouse=True)
def _switches_back(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    yield
    for f in (plan.set_infer_fuse, plan.set_infer_fuse_dwpw, plan.set_infer_fuse_msrb, plan.set_infer_fuse_bneck):
        f(None)


def _model(variant="A", size=256, deployed=False, **kw):
    cfg = litehandnet_cfg(variant, image_size=size, **kw)
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


def _ops(pb):
    cb, cf, cbw, nf, nb = pb.finalize()
    return [bytes(C.string_at(C.addressof(cf[i]), C.sizeof(cf[i]))) for i in range(nf)], cf, nf


def test_both_width_256_classes_are_in_the_table():
    assert {(128, 32), (128, 64), (256, 64), (256, 128)} == set(PlanBuilder.FUSE_BNECK_CHANNELS)


@pytest.mark.parametrize("deployed", [False, True])
@pytest.mark.parametrize("size", [256, 224])
def test_width_256_has_13_bottlenecks(size, deployed):
    pb = _builder(_model(size=size, deployed=deployed, channels=256), size, infer_fuse_bneck=True, **OFF)
    _, cf, nf = _ops(pb)
    fused = [r for r in pb.recs if r["op"] == BNECK]
    assert len(fused) == 13 == pb.n_fused_bneck == sum(cf[i].kind == BNECK for i in range(nf))
    s = size // 4
    assert sorted((r["mids"][0].C, r["x"].H) for r in fused) == sorted(6 * [(64, s // 8)] + 4 * [(64, s // 4)] + 2 * [(64, s // 2)] + [(128, s)])
    assert all(r["x"].C == 256 and r["out"].C == 256 and r["mids"][1].C == r["mids"][0].C and r["mids"][2].C == 256 for r in fused)
    # no BottleNeck-shaped 3x3 is left as a record of its own
    assert not any(r["op"] == KXK and r["x"].C in (64, 128) and r["x"].C == r["out"].C and r["stride"] == 1 for r in pb.recs)
    for i in range(nf):
        if cf[i].kind != BNECK:
            continue
        o = cf[i]
        assert min(o.in_buf) >= 0 and o.in_C[0] == 256 and o.in_C[1] == o.in_C[2] and o.in_C[1] in (64, 128) and o.out_C == 256
        assert o.ws[0] >= pb.table_base and o.ws[0] < pb.table_end and o.ws[1] >= 0
        assert o.p[0] >= 0 and o.p[2] >= 0 and o.p[3] >= 0 and (o.p[1] >= 0) == deployed == (o.p[4] >= 0)
        assert o.f[0] == pytest.approx(0.01)
    # the tap-major scratch slots (9 Cm Cm floats each) lie apart from each other
    slots = sorted((cf[i].ws[1], 36 * cf[i].in_C[1] ** 2) for i in range(nf) if cf[i].kind == BNECK)
    assert all(a + n <= b for (a, n), (b, _) in zip(slots, slots[1:]))


@pytest.mark.parametrize("deployed", [False, True])
@pytest.mark.parametrize("size", [256, 224])
def test_width_256_reduction_2_is_all_cm_128(size, deployed):
    pb = _builder(_model(size=size, deployed=deployed, channels=256, reduction=2), size, infer_fuse_bneck=True, **OFF)
    pb.finalize()
    fused = [r for r in pb.recs if r["op"] == BNECK]
    assert len(fused) == 13 and all((r["x"].C, r["mids"][0].C) == (256, 128) for r in fused)
    s = size // 4
    assert sorted(r["x"].H for r in fused) == sorted(6 * [s // 8] + 4 * [s // 4] + 2 * [s // 2] + [s])


@pytest.mark.parametrize("reduction", [4, 2])
def test_launches_that_leave(reduction):
    m = _model(size=64, channels=256, reduction=reduction)
    off = _builder(m, 64, infer_fuse_bneck=False, **OFF)
    off.finalize()
    on = _builder(m, 64, infer_fuse_bneck=True, **OFF)
    on.finalize()
    n_conv = lambda pb: sum(r["op"] in (PW, KXK) for r in pb.recs)
    n_ew = lambda pb: sum(r["op"] == EW and not r.get("lazy") for r in pb.recs)
    assert n_conv(off) - n_conv(on) == 39 and n_ew(off) - n_ew(on) == 13      # 52 launches become 13
    assert on.act_bytes < off.act_bytes
    for r in (r for r in on.recs if r["op"] == BNECK):
        assert all(on.bufs[t.buf].fused and on.bufs[t.buf].off["data"] == -1 and on.bufs[t.buf].off["table"] >= 0 for t in r["mids"])


def test_training_plans_are_never_rewritten():
    m = _model(size=64, channels=256)
    want = _ops(_builder(m, 64, True, infer_fuse_bneck=False))[0]
    got = _builder(m, 64, True, infer_fuse_bneck=True)
    assert _ops(got)[0] == want and got.n_fused_bneck == 0 and not any(r["op"] == BNECK for r in got.recs)


def test_switch_off_changes_nothing():
    m = _model(channels=256)
    want = _ops(_builder(m, 256))[0]                                 # built without the argument
    new = _builder(m, 256, infer_fuse_bneck=False)
    assert _ops(new)[0] == want and new.n_fused_bneck == 0 and not any(r["op"] == BNECK for r in new.recs)
    assert _ops(_builder(m, 256, infer_fuse_bneck=True))[0] != want


def test_silu_blocks_are_left_alone():
    pb = _builder(_model(channels=256, activation="silu"), 256, infer_fuse_bneck=True, **OFF)
    pb.finalize()
    assert pb.n_fused_bneck == 0 and not any(r["op"] == BNECK for r in pb.recs)


def test_bf16x3_takes_only_what_the_bottlenecks_leave():
    """Both switches on: the inner 3x3s belong to the BNECK launches and stay fp32 -- the rule of width 128."""
    m = _model(channels=256)
    alone = _builder(m, 256, infer_bf16x3=True, **OFF)
    alone.finalize()
    both = _builder(m, 256, infer_fuse_bneck=True, infer_bf16x3=True, **OFF)
    both.finalize()
    assert both.n_fused_bneck == 13 and alone.n_bf16x3 - both.n_bf16x3 == 13
    claimed = {id(c) for r in both.recs if r["op"] == BNECK for c in r["convs"]}
    assert not any(id(r["conv"]) in claimed for r in both.recs if r["op"] in (PW, KXK))


def test_width_128_and_the_hourglass_are_as_before():
    a = _builder(_model(), 256, infer_fuse_bneck=True, **OFF)
    a.finalize()
    assert a.n_fused_bneck == 13 and all(r["x"].C == 128 and r["mids"][0].C in (32, 64) for r in a.recs if r["op"] == BNECK)
    h = _builder(_model("H"), 256, infer_fuse_bneck=True, **OFF)       # C = 256 Residuals: 1x1 -> 3x3 -> 1x1 through pre-activation BatchNorms
    h.finalize()
    assert h.n_fused_bneck == 0 and not any(r["op"] == BNECK for r in h.recs)


# ---------------------------------------------------------------- the kernel cases are not degenerate (float64, reference alone)
SMALL = [k for k, c in bc.CASES.items() if c["n"] <= 5]


def test_case_table_covers_what_it_must():
    for cm in bc.MIDS:
        mine = [c for c in bc.CASES.values() if c["cm"] == cm]
        assert {(1, 5), (2, 3), (4, 4), (7, 7), (8, 8), (14, 14), (16, 16), (9, 70), (24, 40), (12, 70), (9, 11)} <= {(c["h"], c["w"]) for c in mine}
        assert {c["out_slope"] for c in mine} >= {0.0, 0.01, 1.0}
        assert {c["slopes"][:2] for c in mine} >= {(0.0, 0.0), (1.0, 1.0)}
        for j in range(3):
            assert any(not c["tabs"][j] and all(c["tabs"][i] for i in range(3) if i != j) for c in mine)
        for j in range(2):
            assert any(not c["biases"][j] and c["biases"][1 - j] for c in mine)
        assert any(not any(c["tabs"]) and not any(c["biases"]) and not c["const"] for c in mine)
        assert any(c["x"][0] == 512 and c["x"][1] > 0 and c["xtab"] and c["xgate"] for c in mine) and any(c["y"][0] == 512 and c["y"][1] > 0 for c in mine)
        assert {(c["h"], c["w"]) for c in mine if c["shift_far"]} == {(8, 8), (12, 70)}
        assert any(c["n"] * ((c["h"] + 7) // 8) * ((c["w"] + 7) // 8) > 2 * 256 for c in mine)      # more than one resident round
    for name, c in bc.CASES.items():
        assert c["x"][1] + 256 <= c["x"][0] and c["y"][1] + 256 <= c["y"][0], name
        assert 4 * c["n"] * c["h"] * c["w"] * max(c["x"][0], c["y"][0]) <= 9e6, name       # a few MB at the most


@pytest.mark.parametrize("name", SMALL)
def test_case_is_not_degenerate(name):
    """At least 10 % of the pre-activation elements of t1, t2 and of the final sum are negative and at least 10 % positive: every
    slope matters.  Shift-far cases: the reference differs at border pixels from the wrong-padding variant by > 100 floors, and
    nowhere else."""
    c = bc.CASES[name]
    g = bc.inputs(name)
    y, p1, p2, s = bc.reference(name, g, parts=True)
    assert y.shape == (c["n"], c["h"], c["w"], 256) and bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0.1
    for what, p in (("t1", p1), ("t2", p2), ("sum", s)):
        neg, pos = float((p < 0).double().mean()), float((p > 0).double().mean())
        assert neg >= 0.10 and pos >= 0.10, (name, what, neg, pos)
    if c["shift_far"]:
        wrong = bc.reference(name, g, wrong_padding=True)
        b = bc.border(c["h"], c["w"])
        peak = float(y.abs().max())
        d_border = float((wrong - y)[:, b].abs().max()) / peak
        assert d_border > 100 * bc.FLOOR, (name, d_border)
        assert float((wrong - y)[:, ~b].abs().max()) < 1e-9 * peak
    if c["const"]:
        assert float((y - bc.const_answer(name)).abs().max()) < 1e-7      # (1 / (9 Cm) is rounded to float32 in the inputs)
