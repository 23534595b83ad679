"""CPU: the depthwise -> 1x1 inference fusion pass of the plan compiler (PlanBuilder.fuse_dw_pw, switched by
LHN_INFER_FUSE_DWPW=1 or plan.set_infer_fuse_dwpw) -- no GPU, no kernel launch.  A pair is a 3x3 depthwise convolution (stride 1,
padding == dilation in {1, 2}, 32 or 64 channels, one source) whose whole, ungated output buffer is read by nothing but one
stride-1 1x1 over all of it with 32 or 64 output channels; the tests find the pairs in the switch-off plan by that rule, written
out here independently of the pass."""
import ctypes as C
import os
import re

import pytest

from litehandnet_amd import _lib, get_model, plan
from litehandnet_amd.config import litehandnet_cfg
from litehandnet_amd.liteHandNet import DWConv
from litehandnet_amd.plan import DW, DWPW, FINALIZE, PW, PWDW, TABLE_FILL, PlanBuilder, TCat, TRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _switches_back():
    plan.set_infer_fuse(None)
    plan.set_infer_fuse_dwpw(None)
    yield
    plan.set_infer_fuse(None)
    plan.set_infer_fuse_dwpw(None)


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


def _dw_pw_pairs(pb):
    """(depthwise record, 1x1 record) pairs of an unfused plan, by the rule in the module docstring."""
    io = {v.buf for v in (pb.in_ref, pb.out_ref) if v is not None}
    out = []
    for q in pb.recs:
        if q["op"] != DW or q["k"] != 3 or q["stride"] != 1 or q["pad"] != q["dil"] or q["dil"] not in (1, 2):
            continue
        if q["conv"].weight is None or q.get("bn_repeat", 1) != 1 or q.get("xs") is not None:
            continue
        x, t = q["x"], q["out"]
        b = pb.bufs[t.buf]
        if x.buf < 0 or x.C not in (32, 64) or t.coff != 0 or b.C != t.C or b.gate or b.lazy is not None or t.buf in io:
            continue
        if q["bn"] is not None and q["conv"].bias is not None:
            continue
        readers = [r for r in pb.recs if r is not q and r["op"] != TABLE_FILL and
                   any(v.buf == t.buf for val in r.values() for v in _views(val))]
        if len(readers) != 1:
            continue
        r = readers[0]
        if r["op"] != PW or r["stride"] != 1 or r["nchw"] or r["wrc"] != (0, 0) or r["bn_repeat"] != 1 or r.get("xs") is not None:
            continue
        y = r["out"]
        if (r["x"].buf, r["x"].coff, r["x"].C) != (t.buf, 0, t.C) or y.C not in (32, 64) or y.buf == t.buf:
            continue
        if r["bn"] is not None and r["conv"].bias is not None:
            continue
        if y.buf == x.buf and x.coff < y.coff + y.C and y.coff < x.coff + x.C:
            continue
        out.append((q, r))
    return out


def _pw_dw_pairs(pb):
    """(1x1 record, depthwise record) pairs the OLD rule accepts (tests/test_infer_fuse_cpu.py: _pairs)."""
    out = []
    for r in pb.recs:
        if r["op"] != PW or r["stride"] != 1 or r["nchw"] or r["x"].buf < 0:
            continue
        t = r["out"]
        if r["x"].C != 64 or t.C != 64 or t.coff != 0 or pb.bufs[t.buf].C != t.C:
            continue
        readers = [q for q in pb.recs if q is not r and q["op"] != TABLE_FILL and
                   any(v.buf == t.buf for val in q.values() for v in _views(val))]
        if len(readers) == 1 and readers[0]["op"] == DW and (readers[0]["k"], readers[0]["stride"], readers[0]["pad"], readers[0]["dil"]) == (3, 1, 1, 1) \
                and (readers[0]["x"].buf, readers[0]["x"].coff, readers[0]["x"].C) == (t.buf, 0, t.C):
            out.append((r, readers[0]))
    return out


def _ops(pb):
    cb, cf, cbw, nf, nb = pb.finalize()
    return [bytes(C.string_at(C.addressof(cf[i]), C.sizeof(cf[i]))) for i in range(nf)], cb


def _key(x, y):
    return (x.buf, x.coff, x.C, y.buf, y.coff, y.C)


@pytest.mark.parametrize("deployed", [False, True])
def test_variant_a_pairs_are_fused(deployed):
    cfg = litehandnet_cfg("A", image_size=256)
    cfg.MODEL["ca_dropout"] = 0.0
    m = get_model(cfg)
    if deployed:                                                     # the deployed module tree, built without the GPU fold
        from torch import nn
        for u in m.modules():
            if hasattr(u, "conv") and hasattr(u, "slope") and not hasattr(u, "rep_conv"):
                c = u.conv.conv
                u.rep_conv = nn.Conv2d(c.in_channels, c.out_channels, c.kernel_size, c.stride, c.padding, c.dilation, c.groups, bias=True)
                del u.conv
            if hasattr(u, "rbr_dense"):
                c = u.rbr_dense.conv
                u.rbr_reparam = nn.Conv2d(c.in_channels, c.out_channels, c.kernel_size, c.stride, c.padding, c.dilation, c.groups, bias=True)
                del u.rbr_dense, u.rbr_1x1
                if hasattr(u, "rbr_identity"):
                    del u.rbr_identity
    off = _builder(m, 2, 256, False, infer_fuse=False, infer_fuse_dwpw=False)
    pairs = _dw_pw_pairs(off)
    assert len(pairs) == 16                                          # 2 MSABs x 8 DWConv
    assert sorted((q["x"].C, r["out"].C, q["dil"]) for q, r in pairs) == sorted(
        2 * [(64, 32, 1), (32, 32, 1), (64, 32, 2), (32, 32, 1), (64, 64, 1), (64, 64, 1), (64, 64, 2), (64, 64, 1)])
    plan.set_infer_fuse_dwpw(True)
    on = _builder(m, 2, 256, False)
    assert on.infer_fuse_dwpw and not on.infer_fuse
    _, cb = _ops(on)
    fused = [r for r in on.recs if r["op"] == DWPW]
    assert len(fused) == len(pairs) == on.n_fused_dwpw and on.n_fused == 0
    assert sorted(_key(r["x"], r["out"]) + (r["dil"],) for r in fused) == sorted(_key(q["x"], r["out"]) + (q["dil"],) for q, r in pairs)
    assert not _dw_pw_pairs(on)
    for kind in (PW, DW):
        assert sum(r["op"] == kind for r in on.recs) == sum(r["op"] == kind for r in off.recs) - len(pairs)
    off.finalize()
    for r in fused:                                                  # the tensor in between has a table and no data
        b = on.bufs[r["mid"].buf]
        assert b.fused and b.off["data"] == -1 and cb[r["mid"].buf].data_off == -1 and b.off["table"] >= 0
        assert not any(v.buf == r["mid"].buf for q in on.recs if q["op"] not in (DWPW, FINALIZE, TABLE_FILL)
                       for val in q.values() for v in _views(val))
    saved = sum(2 * b.H * b.W * b.C * 4 for b in on.bufs if b.fused)
    assert off.total_bytes - on.total_bytes >= saved > 0
    fin = [r for r in on.recs if r["op"] == FINALIZE]
    mids = {r["mid"].buf for r in fused}
    if deployed:                                                     # the depthwise bias / activation: the TABLE_FILL that was there
        assert not fin
        fills = [r for r in on.recs if r["op"] == TABLE_FILL and r["out"].buf in mids]
        assert len(fills) == len(fused) and all(r["bias"] is not None for r in fills)
        for r in fused:
            assert r["bias"] is r["conv2"].bias is not None
            pos = {id(q): i for i, q in enumerate(on.recs)}
            assert max(pos[id(f)] for f in fills if f["out"].buf == r["mid"].buf) < pos[id(r)]
    else:                                                            # eval: both BatchNorm tables from running statistics
        assert len(fin) == 2 * len(fused) and all(r["bias"] is None for r in fused)
        assert {(r["out"].buf, r["out"].coff) for r in fin} == {(b, 0) for b in mids} | {(r["out"].buf, r["out"].coff) for r in fused}


def test_both_switches_on():
    off = _model("A", infer_fuse=False, infer_fuse_dwpw=False)
    pairs = _dw_pw_pairs(off)
    old = _pw_dw_pairs(off)
    assert len(old) >= 4
    on = _model("A", infer_fuse=True, infer_fuse_dwpw=True)
    on.finalize()
    dwpw = [r for r in on.recs if r["op"] == DWPW]
    pwdw = [r for r in on.recs if r["op"] == PWDW]
    assert len(dwpw) == len(pairs) == on.n_fused_dwpw == 16          # the new pass claims its pairs first
    assert on.n_fused == len(pwdw)
    claimed = [id(c) for r in dwpw + pwdw for c in (r["conv"], r["conv2"])]
    assert len(claimed) == len(set(claimed))                         # no convolution is claimed twice
    old_keys = {(id(p["conv"]), id(q["conv"])) for p, q in old}
    assert all((id(r["conv"]), id(r["conv2"])) in old_keys for r in pwdw)
    for kind in (PW, DW):
        assert sum(r["op"] == kind for r in on.recs) == sum(r["op"] == kind for r in off.recs) - len(dwpw) - len(pwdw)


def test_switch_off_changes_nothing(monkeypatch):
    monkeypatch.delenv("LHN_INFER_FUSE_DWPW", raising=False)
    monkeypatch.delenv("LHN_INFER_FUSE", raising=False)
    for fuse in (False, True):
        class Old(PlanBuilder):                                      # a builder that never heard of the switch
            def fuse_dw_pw(self):
                return 0
        cfg = litehandnet_cfg("A", image_size=256)
        cfg.MODEL["ca_dropout"] = 0.0
        m = get_model(cfg)
        tensors = list(m.state_dict(keep_vars=True).values())
        old = Old(2, {id(t): j for j, t in enumerate(tensors)}, image_hw=(256, 256), with_backward=False, p_drop=0.0, infer_fuse=fuse)
        m.emit(old, old.image())
        want, _ = _ops(old)
        new = _builder(m, 2, 256, False, infer_fuse=fuse)
        assert not new.infer_fuse_dwpw
        plain, _ = _ops(new)
        assert plain == want and new.n_fused_dwpw == 0 and not any(r["op"] == DWPW for r in new.recs)
        explicit, _ = _ops(_builder(m, 2, 256, False, infer_fuse=fuse, infer_fuse_dwpw=False))
        assert explicit == want
        plan.set_infer_fuse_dwpw(True)
        plan.set_infer_fuse_dwpw(False)
        assert _ops(_builder(m, 2, 256, False, infer_fuse=fuse))[0] == want
        plan.set_infer_fuse_dwpw(None)
    monkeypatch.setenv("LHN_INFER_FUSE_DWPW", "1")
    assert plan.infer_fuse_dwpw_enabled() and not plan.infer_fuse_enabled()
    pb = _model("A")
    assert pb.infer_fuse_dwpw and not pb.infer_fuse
    assert _ops(pb)[0] != want


@pytest.mark.parametrize("variant", ["A", "B", "M"])
def test_training_plans_are_never_rewritten(variant):
    plan.set_infer_fuse_dwpw(False)
    ops_want, _ = _ops(_model(variant, backward=True))
    plan.set_infer_fuse_dwpw(True)
    got = _model(variant, backward=True)
    ops_got, _ = _ops(got)
    assert got.n_fused_dwpw == 0 and not any(r["op"] == DWPW for r in got.recs)
    assert ops_got == ops_want


def test_unaccepted_unit_keeps_its_two_ops():
    plan.set_infer_fuse_dwpw(True)
    pb = _builder(DWConv(40, 40), 2, 16, False, image=False, cin=40)
    pb.finalize()
    assert pb.n_fused_dwpw == 0 and not any(r["op"] == DWPW for r in pb.recs)
    assert sum(r["op"] == PW for r in pb.recs) == 1 and sum(r["op"] == DW and r["k"] == 3 for r in pb.recs) == 1
    pb = _builder(DWConv(64, 32, dilation=2, padding=2), 2, 16, False, image=False, cin=64)      # the same unit at 64 -> 32 is taken
    pb.finalize()
    assert pb.n_fused_dwpw == 1 and [r["dil"] for r in pb.recs if r["op"] == DWPW] == [2]
    pb = _builder(DWConv(64, 64, dilation=3, padding=3), 2, 16, False, image=False, cin=64)      # dilation 3 is not
    pb.finalize()
    assert pb.n_fused_dwpw == 0


def test_symbol_is_declared_listed_and_exported():
    with open(os.path.join(ROOT, "include", "lhn.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+lhn_conv_dw3_pw_fwd\s*\(", header)
    assert "lhn_conv_dw3_pw_fwd" in _lib.SYMBOLS
    so = C.CDLL(_lib.LIB_PATH)
    assert hasattr(so, "lhn_conv_dw3_pw_fwd")
    assert _lib.lib().lhn_conv_dw3_pw_fwd.argtypes is not None and len(_lib.lib().lhn_conv_dw3_pw_fwd.argtypes) == 8
    assert _lib.lib().lhn_version() == 3
