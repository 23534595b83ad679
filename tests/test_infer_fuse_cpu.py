"""CPU: the inference fusion pass of the plan compiler (PlanBuilder.fuse_pw_dw, switched by LHN_INFER_FUSE=1 or
plan.set_infer_fuse) -- no GPU, no kernel launch.  A pair is a 64 -> 64 stride-1 1x1 whose output buffer is read by nothing but
one 3x3 depthwise convolution (stride 1, dilation 1, padding 1) over all of it; the tests find the pairs in the switch-off plan
by that rule, written out here independently of the pass."""
import ctypes as C
from collections import Counter

import pytest

from litehandnet_amd import get_model, plan
from litehandnet_amd.config import litehandnet_cfg
from litehandnet_amd.litehourglass import RepBasicUnit
from litehandnet_amd.plan import DW, FINALIZE, PW, PWDW, TABLE_FILL, PlanBuilder, TCat, TRef


@pytest.fixture(autouse=True)
def _switch_back():
    yield
    plan.set_infer_fuse(None)


def _builder(m, n, size, backward, image=True, cin=None, **kw):
    tensors = list(m.state_dict(keep_vars=True).values())
    pb = PlanBuilder(n, {id(t): j for j, t in enumerate(tensors)}, image_hw=(size, size), with_backward=backward, p_drop=0.0, **kw)
    y = m.emit(pb, pb.image() if image else pb.input_tensor(cin, size, size))
    if getattr(y, "buf", None) != -2:
        pb.set_output(y)
    return pb


def _model(variant, size=256, backward=False, n=2, **kw):
    cfg = litehandnet_cfg(variant, image_size=size)
    cfg.MODEL["ca_dropout"] = 0.0
    return _builder(get_model(cfg), n, size, backward, **kw)


def _views(v):
    if isinstance(v, TRef):
        return [v]
    if isinstance(v, TCat):
        return list(v.parts)
    if isinstance(v, (list, tuple)):
        return [t for u in v for t in _views(u)]
    return []


def _pairs(pb, channels=(64,)):
    """(1x1 record, depthwise record) pairs of an unfused plan, by the rule in the module docstring."""
    out = []
    for r in pb.recs:
        if r["op"] != PW or r["stride"] != 1 or r["nchw"] or r["x"].buf < 0:
            continue
        t = r["out"]
        if r["x"].C not in channels or t.C != r["x"].C or t.coff != 0 or pb.bufs[t.buf].C != t.C:
            continue
        readers = [q for q in pb.recs if q is not r and q["op"] != TABLE_FILL and
                   any(v.buf == t.buf for key, val in q.items() for v in _views(val))]
        if len(readers) != 1:
            continue
        q = readers[0]
        if q["op"] == DW and (q["k"], q["stride"], q["pad"], q["dil"]) == (3, 1, 1, 1) and (q["x"].buf, q["x"].coff, q["x"].C) == (t.buf, 0, t.C):
            out.append((r, q))
    return out


def _ops(pb):
    cb, cf, cbw, nf, nb = pb.finalize()
    return [bytes(C.string_at(C.addressof(cf[i]), C.sizeof(cf[i]))) for i in range(nf)], cb


def test_variant_b_pairs_are_fused():
    off = _model("B", infer_fuse=False)
    pairs = _pairs(off)
    by_level = Counter(r["x"].H for r, _ in pairs)
    assert 12 <= len(pairs) <= 24 and set(by_level) == {64, 32, 16, 8}, by_level       # (counted by hand: 18 = 6 / 4 / 4 / 4)
    plan.set_infer_fuse(True)
    on = _model("B")
    _, cb = _ops(on)
    fused = [r for r in on.recs if r["op"] == PWDW]
    assert len(fused) == len(pairs) == on.n_fused
    assert Counter(r["x"].H for r in fused) == by_level
    assert sorted((r["x"].buf, r["x"].coff, r["out"].buf, r["out"].coff) for r in fused) == \
        sorted((p["x"].buf, p["x"].coff, q["out"].buf, q["out"].coff) for p, q in pairs)
    assert not _pairs(on)                                            # no 1x1 / depthwise op is left for those pairs
    assert sum(r["op"] == PW for r in on.recs) == sum(r["op"] == PW for r in off.recs) - len(pairs)
    assert sum(r["op"] == DW for r in on.recs) == sum(r["op"] == DW for r in off.recs) - len(pairs)
    off.finalize()
    for r in fused:                                                  # the tensor in between has a table and no data
        b = on.bufs[r["mid"].buf]
        assert b.fused and b.off["data"] == -1 and cb[r["mid"].buf].data_off == -1 and b.off["table"] >= 0
        assert not any(v.buf == r["mid"].buf for q in on.recs if q["op"] not in (PWDW, FINALIZE, TABLE_FILL)
                       for val in q.values() for v in _views(val))
    saved = sum(2 * b.H * b.W * b.C * 4 for b in on.bufs if b.fused)
    assert off.total_bytes - on.total_bytes >= saved > 0
    # eval form: both BatchNorm tables are still built (from running statistics), by launches the table cache can skip
    fin = [r for r in on.recs if r["op"] == FINALIZE]
    assert len(fin) == 2 * len(fused)
    assert {(r["out"].buf, r["out"].coff) for r in fin} == {(r["mid"].buf, 0) for r in fused} | {(r["out"].buf, r["out"].coff) for r in fused}


def test_switch_off_changes_nothing(monkeypatch):
    monkeypatch.delenv("LHN_INFER_FUSE", raising=False)
    plain, _ = _ops(_model("B"))                                     # default: off
    assert not any(r["op"] in (PWDW, FINALIZE) for r in _model("B").recs)
    explicit, _ = _ops(_model("B", infer_fuse=False))
    assert plain == explicit
    plan.set_infer_fuse(True)
    plan.set_infer_fuse(False)
    again, _ = _ops(_model("B"))
    assert plain == again
    monkeypatch.setenv("LHN_INFER_FUSE", "1")
    plan.set_infer_fuse(None)
    assert _model("B").infer_fuse and plan.infer_fuse_enabled()
    assert _ops(_model("B"))[0] != plain


@pytest.mark.parametrize("variant", ["A", "B", "M"])
def test_training_plans_are_never_rewritten(variant):
    plan.set_infer_fuse(False)
    want = _model(variant, backward=True)
    ops_want, _ = _ops(want)
    plan.set_infer_fuse(True)
    got = _model(variant, backward=True)
    ops_got, _ = _ops(got)
    assert got.n_fused == 0 and not any(r["op"] == PWDW for r in got.recs)
    assert ops_got == ops_want


@pytest.mark.parametrize("variant", ["A", "M"])
def test_other_variants_fuse_their_64_pairs_only(variant):
    off = _model(variant, infer_fuse=False)
    pairs = _pairs(off)
    assert len(pairs) >= 4
    on = _model(variant, infer_fuse=True)
    on.finalize()
    fused = [r for r in on.recs if r["op"] == PWDW]
    assert len(fused) == len(pairs) and all(r["x"].C == 64 and r["out"].C == 64 for r in fused)
    for kind in (PW, DW):                                            # every other 1x1 / depthwise (the 64 -> 32 pairs too) keeps its op
        assert sum(r["op"] == kind for r in on.recs) == sum(r["op"] == kind for r in off.recs) - len(pairs)


def test_unaccepted_unit_keeps_its_two_ops():
    plan.set_infer_fuse(True)
    pb = _builder(RepBasicUnit(40, 40, "none"), 2, 16, False, image=False, cin=40)
    pb.finalize()
    assert pb.n_fused == 0 and not any(r["op"] == PWDW for r in pb.recs)
    assert sum(r["op"] == PW for r in pb.recs) >= 1 and sum(r["op"] == DW and r["k"] == 3 for r in pb.recs) >= 1
    pb = _builder(RepBasicUnit(128, 128, "none"), 2, 16, False, image=False, cin=128)      # the same unit at 64 + 64 channels is taken
    pb.finalize()
    assert pb.n_fused == 1
