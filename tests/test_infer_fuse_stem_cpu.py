"""CPU: the stem inference fusion pass of the plan compiler (PlanBuilder.fuse_stem, switched by LHN_INFER_FUSE_STEM=1 or
plan.set_infer_fuse_stem) -- no GPU, no kernel launch -- and the non-degeneracy of the kernel cases of tests/stem_tail_cases.py
(float64 only).  The pattern: a MAXPOOL of a whole fresh 32-channel buffer t into channels [32, 64) of a 64-channel buffer, a plain
1x1 (32 -> 32) reading t, its sole reader a 3x3 (stride 2, pad 1) into channels [0, 32), and the sole reader of the 64 channels a plain
1x1 (64 -> 128); t's writer is absorbed when it is a plain depthwise 3x3 / 7x7."""
import ctypes as C
import os
import re

import pytest
import torch

import stem_tail_cases as sc
from litehandnet_amd import _lib, get_model, plan
from litehandnet_amd.config import litehandnet_cfg
from litehandnet_amd.plan import BNECK, DW, FINALIZE, KXK, MAXPOOL, PW, STEMTAIL, TABLE_FILL, PlanBuilder
from test_infer_fuse_bneck_cpu import _deploy_without_gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("LHN_INFER_FUSE_STEM", "LHN_INFER_BF16X3", "LHN_INFER_FUSE_BNECK", "LHN_INFER_FUSE_MSRB", "LHN_INFER_FUSE_DWPW", "LHN_INFER_FUSE")
SETTERS = (plan.set_infer_fuse, plan.set_infer_fuse_dwpw, plan.set_infer_fuse_msrb, plan.set_infer_fuse_bneck, plan.set_infer_bf16x3,
           plan.set_infer_fuse_stem)
OFF = dict(infer_fuse=False, infer_fuse_dwpw=False, infer_fuse_msrb=False)


@pytest.fixture(autouse=True)
def _switches_back(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    yield
    for f in SETTERS:
        f(None)


def _model(variant="A", size=64, deployed=False, **kw):
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


@pytest.mark.parametrize("variant,deployed,K", [("A", False, 0), ("A", True, 7), ("M", False, 3)])
def test_one_stemtail_record_replaces_the_stem(variant, deployed, K):
    m = _model(variant, 64, deployed)
    off = _builder(m, 64, **OFF)
    off.finalize()
    on = _builder(m, 64, infer_fuse_stem=True, **OFF)
    _, cf, nf = _ops(on)
    fused = [r for r in on.recs if r["op"] == STEMTAIL]
    assert len(fused) == 1 == on.n_fused_stem == sum(cf[i].kind == STEMTAIL for i in range(nf)) and off.n_fused_stem == 0
    r = fused[0]
    j = next(i for i, q in enumerate(on.recs) if q is r)
    assert r["K"] == K and (r["x"].H, r["x"].W, r["x"].C) == (32, 32, 32) and (r["out"].H, r["out"].W, r["out"].C) == (16, 16, 128)
    assert (r["dw"] is not None) == (K > 0) and ((r["x"].buf == r["t"].buf) == (K == 0))
    # none of the records it replaced is left: the stem's max pool, the stride-2 3x3 and every convolution touching t / u / cat
    inner = {r["u"].buf, r["cat"].buf} | ({r["t"].buf} if K else set())
    assert not any(q["op"] == MAXPOOL and q["x"].buf == r["t"].buf for q in on.recs)
    s2 = lambda pb: [q for q in pb.recs if q["op"] == KXK and q["stride"] == 2 and (q["x"].H, q["x"].C, q["out"].C) == (32, 32, 32)]
    assert not s2(on) and len(s2(off)) == 1
    for q in on.recs:
        if q is r or q["op"] in (FINALIZE, TABLE_FILL):
            continue
        assert not any(v.buf in inner for val in q.values() for v in plan._refs_in(val)), q["op"]
    if K:
        assert not any(q["op"] == DW and q["k"] == K and q["x"].C == 32 and q["x"].H == 32 for q in on.recs)
    # table-only buffers, filled ahead of the launch by what fills them in the unfused plan
    for b in inner:
        assert on.bufs[b].fused and on.bufs[b].off["data"] == -1 and on.bufs[b].off["table"] >= 0
        fills = [i for i, q in enumerate(on.recs) if q["op"] in (FINALIZE, TABLE_FILL) and q["out"].buf == b]
        # (deployed A: branch1's 1x1 adds its bias while storing and has slope 1 -- nothing is pending in u's table)
        assert len(fills) == (0 if deployed and b == r["u"].buf else 1) and all(i < j for i in fills)
        assert all(on.recs[i]["op"] == (TABLE_FILL if deployed else FINALIZE) and on.recs[i]["out"].C == 32 for i in fills)
    assert (not on.bufs[r["t"].buf].fused) == (K == 0)
    assert on.act_bytes < off.act_bytes
    # the op
    o = next(cf[i] for i in range(nf) if cf[i].kind == STEMTAIL)
    assert o.i[0] == K and o.i[1] == 64 and list(o.in_C) == [32, 32, 32] and o.out_C == 128 and min(o.in_buf) >= 0
    assert on.table_base <= o.ws[0] < on.table_end and o.ws[0] == on.bufs[r["cat"].buf].off["table"] and o.ws[1] >= 0
    assert (o.p[0] >= 0) == (K > 0) and o.p[2] >= 0 and o.p[4] >= 0 and o.p[6] >= 0 and o.p[7] >= 0
    # biases: a 1x1 without BatchNorm adds its own (deployed b1, always b3); mynet's branch1 has biases in front of its BatchNorms
    assert (o.p[3] >= 0) == (deployed or variant == "M") and (o.p[5] >= 0) == (variant == "M") and o.p[1] < 0
    n_ops = lambda pb: sum(q["op"] in (PW, KXK, DW, MAXPOOL) for q in pb.recs)
    assert n_ops(off) - n_ops(on) == (5 if K else 4)


@pytest.mark.parametrize("variant,kw", [("B", {}), ("A", {"input_channel": 256}), ("A", {"activation": "silu"})])
def test_other_stems_are_left_alone(variant, kw):
    m = _model(variant, 64, **kw)
    want = _ops(_builder(m, 64, **OFF))[0]
    on = _builder(m, 64, infer_fuse_stem=True, **OFF)
    assert _ops(on)[0] == want and on.n_fused_stem == 0 and not any(r["op"] == STEMTAIL for r in on.recs)


@pytest.mark.parametrize("variant,deployed", [("A", False), ("A", True), ("M", False)])
def test_switch_off_or_backward_changes_nothing(variant, deployed):
    m = _model(variant, 64, deployed)
    want = _ops(_builder(m, 64))[0]                                  # built without the argument
    new = _builder(m, 64, infer_fuse_stem=False)
    assert _ops(new)[0] == want and new.n_fused_stem == 0 and not any(r["op"] == STEMTAIL for r in new.recs)
    assert _ops(_builder(m, 64, infer_fuse_stem=True))[0] != want
    if not deployed:
        want_b = _builder(m, 64, True)
        ops_b, _, _ = _ops(want_b)
        got = _builder(m, 64, True, infer_fuse_stem=True)
        cb, cf, cbw, nf, nb = got.finalize()
        assert [bytes(C.string_at(C.addressof(cf[i]), C.sizeof(cf[i]))) for i in range(nf)] == ops_b
        assert got.n_fused_stem == 0 and not any(r["op"] == STEMTAIL for r in got.recs)


def test_pass_runs_first_and_leaves_the_others_alone():
    m = _model("A", 256)
    five = dict(infer_fuse=True, infer_fuse_dwpw=True, infer_fuse_msrb=True, infer_fuse_bneck=True, infer_bf16x3=True)
    a = _builder(m, 256, **five)
    a.finalize()
    b = _builder(m, 256, infer_fuse_stem=True, **five)
    b.finalize()
    assert (a.n_fused, a.n_fused_dwpw, a.n_fused_msrb, a.n_fused_bneck, a.n_bf16x3) == (b.n_fused, b.n_fused_dwpw, b.n_fused_msrb, b.n_fused_bneck, b.n_bf16x3)
    assert b.n_fused_stem == 1 and a.n_fused_stem == 0 and b.n_fused_bneck == 13
    assert [id(c) for r in a.recs if r["op"] == BNECK for c in r["convs"]] == [id(c) for r in b.recs if r["op"] == BNECK for c in r["convs"]]


def test_set_none_falls_back_to_the_environment(monkeypatch):
    m = _model("A", 64)
    assert not plan.infer_fuse_stem_enabled()
    plan.set_infer_fuse_stem(True)
    assert plan.infer_fuse_stem_enabled() and _builder(m, 64, infer_fuse_stem=None).infer_fuse_stem
    plan.set_infer_fuse_stem(False)
    monkeypatch.setenv("LHN_INFER_FUSE_STEM", "1")
    assert not plan.infer_fuse_stem_enabled()
    plan.set_infer_fuse_stem(None)
    assert plan.infer_fuse_stem_enabled() and not plan.infer_fuse_bneck_enabled() and not plan.infer_bf16x3_enabled()
    pb = _builder(m, 64, infer_fuse_stem=None)
    pb.finalize()
    assert pb.infer_fuse_stem and pb.n_fused_stem == 1
    assert not _builder(m, 64).infer_fuse_stem                       # the argument's default is off, whatever the environment says


def test_plan_key_has_the_flag_ahead_of_bf16x3():
    """Engine.plan_for: (shape, backward, p_drop, device, fuse_stem, bf16x3, bneck, msrb, dwpw, fuse) -- the new flag at index 4, so the
    keys callers index from the end (k[-5:]) keep their meaning.  Read from the source: building a plan needs the GPU."""
    with open(os.path.join(ROOT, "litehandnet_amd", "engine.py")) as f:
        src = f.read()
    key = re.search(r"key = \(([^\n]*)\)\n", src).group(1)
    names = [s.strip() for s in key.split(",")]
    assert names.index("fuse_stem") == 4 and names[5:] == ["bf16x3", "fuse_bneck", "fuse_msrb", "fuse_dwpw", "fuse"]
    assert "infer_fuse_stem=fuse_stem" in src and "infer_fuse_stem_enabled() and not with_backward and (deployed or not self.module.training)" in src


def test_symbol_is_declared_listed_and_exported():
    with open(os.path.join(ROOT, "include", "lhn.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+lhn_stem_tail_fwd\s*\(", header)
    assert "liteHandNet.py:169-193" in header and "models/pose_hg_ms_att.py:196-228" in header
    so = C.CDLL(_lib.LIB_PATH)
    assert "lhn_stem_tail_fwd" in _lib.SYMBOLS and hasattr(so, "lhn_stem_tail_fwd")
    L = _lib.lib()
    assert len(L.lhn_stem_tail_fwd.argtypes) == 16 and L.lhn_version() == 3
    assert STEMTAIL == BNECK + 1


# ---------------------------------------------------------------- the kernel cases are not degenerate (float64, reference alone)
SMALL = [k for k, c in sc.CASES.items() if c["n"] <= 5 and c["h"] * c["w"] <= 1600]


def test_case_table_covers_what_it_must():
    for k in sc.KS:
        mine = {n: c for n, c in sc.CASES.items() if c["k"] == k}
        sizes = {(c["h"], c["w"]) for c in mine.values()}
        assert {(1, 1), (1, 5), (2, 3), (3, 3), (7, 7), (8, 8), (16, 16), (17, 17), (18, 18), (28, 28), (9, 70), (24, 40), (37, 19), (12, 70),
                (112, 112)} <= sizes
        assert {c["slopes"] for c in mine.values()} >= {(0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.01, 0.01, 0.01)}
        for j in range(3):
            assert any(not c["tabs"][j] and all(c["tabs"][i] for i in range(3) if i != j) for c in mine.values())
        for j in range(4):
            assert any(not c["biases"][j] and all(c["biases"][i] for i in range(4) if i != j) for c in mine.values())
        assert any(not any(c["tabs"]) and not any(c["biases"]) for c in mine.values())
        assert {(c["h"], c["w"]) for c in mine.values() if c["shift_far"]} == {(8, 8), (17, 17), (12, 70)}
        assert any(c["mixed"] for c in mine.values()) and any(c["pool_negative"] and (c["h"], c["w"]) == (17, 17) for c in mine.values())
        assert any(c["x"] == (256, 64) and c["xtab"] and c["xgate"] for c in mine.values()) and any(c["y"][0] == 256 for c in mine.values())
        assert any(c["xshift_far"] for c in mine.values()) == (k > 0)
        assert any(c["n"] > 768 and (c["h"], c["w"]) == (4, 4) for c in mine.values())      # more workgroups than one resident round
        for name, c in mine.items():
            assert 2 <= c["n"] <= 5 or name.startswith("multi_round"), name
            assert c["x"][1] + 32 <= c["x"][0] and c["y"][1] + 128 <= c["y"][0], name


@pytest.mark.parametrize("name", SMALL)
def test_case_is_not_degenerate(name):
    """Finite, non-trivial output; where a slope is neither 1 nor absent, at least 10 % of the pre-activations on either side of 0.
    Each guarding case: the wrong-arithmetic variant it guards against differs from the reference by more than 100 floors."""
    c = sc.CASES[name]
    g = sc.inputs(name)
    y, pt, pu, pv, t = sc.reference(name, g, parts=True)
    oh, ow = (c["h"] + 1) // 2, (c["w"] + 1) // 2
    assert y.shape == (c["n"], oh, ow, 128) and bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0.1
    peak = float(y.abs().max())
    plain = not (c["shift_far"] or c["pool_negative"] or c["xshift_far"]) and c["h"] * c["w"] >= 9
    for what, p, j in (("t", pt, 0), ("u", pu, 1), ("v", pv, 2)):
        if p is not None and plain and c["tabs"][j]:
            neg, pos = float((p < 0).double().mean()), float((p > 0).double().mean())
            assert neg >= 0.10 and pos >= 0.10, (name, what, neg, pos)
    diff = lambda wrong: (sc.reference(name, g, wrong=wrong) - y).abs()
    if c["shift_far"]:
        d = diff("u_pad")
        assert float(d[:, 0].max()) / peak > 100 * sc.FLOOR and float(d[:, :, 0].max()) / peak > 100 * sc.FLOOR, name
        if oh > 2 and ow > 2:                                            # and only at the border
            assert float(d[:, ~sc.border(oh, ow)].max()) < 1e-9 * peak
    if c["xshift_far"]:
        d = diff("x_pad")
        assert float(d[:, sc.border(oh, ow)].max()) / peak > 100 * sc.FLOOR, name
    if c["pool_negative"]:
        assert float(t.max()) < 0 and c["h"] % 2 == 1 and c["w"] % 2 == 1
        d = diff("pool_zero")
        assert float(d[:, -1].max()) / peak > 100 * sc.FLOOR and float(d[:, :, -1].max()) / peak > 100 * sc.FLOOR, name
        assert float(d[:, :-1, :-1].max()) < 1e-9 * peak
    if c["mixed"]:
        assert float(diff("table_after_max").max()) / peak > 100 * sc.FLOOR, name
