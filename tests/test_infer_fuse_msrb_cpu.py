"""CPU: the MSRB-round inference fusion pass of the plan compiler (PlanBuilder.fuse_msrb_round, switched by LHN_INFER_FUSE_MSRB=1 or
plan.set_infer_fuse_msrb) -- no GPU, no kernel launch.  A round is a pair of 3x3 depthwise convolutions (stride 1, padding ==
dilation, one at dilation 1 and one at dilation 2, the same channel count in {32, 64, 128}, at most two summed sources each) whose
outputs are the lower and the upper half of one whole buffer that nothing else writes and that is neither the plan's input nor
its output; a ChannelAttension / SEBlock that gates that buffer hands its pooling launch to the fused record.  The tests find
the rounds in the switch-off plan by that rule, written out here independently of the pass."""
import ctypes as C
import itertools
import os
import re

import pytest
from torch import nn

from litehandnet_amd import _lib, get_model, plan
from litehandnet_amd.config import litehandnet_cfg
from litehandnet_amd.litehourglass import MSRB as MSRBModule
from litehandnet_amd.plan import AVGPOOL, CA_MLP, DW, DWPW, FINALIZE, MSRB, PW, PWDW, SE_MLP, TABLE_FILL, PlanBuilder, TCat, TRef
from plan_digest import _deploy_without_gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _switches_back():
    for f in (plan.set_infer_fuse, plan.set_infer_fuse_dwpw, plan.set_infer_fuse_msrb):
        f(None)
    yield
    for f in (plan.set_infer_fuse, plan.set_infer_fuse_dwpw, plan.set_infer_fuse_msrb):
        f(None)


def _builder(m, n, size, backward, image=True, cin=None, cls=PlanBuilder, **kw):
    tensors = list(m.state_dict(keep_vars=True).values())
    pb = cls(n, {id(t): j for j, t in enumerate(tensors)}, image_hw=(size, size), with_backward=backward, p_drop=0.0, **kw)
    y = m.emit(pb, pb.image() if image else pb.input_tensor(cin, size, size))
    if getattr(y, "buf", None) != -2:
        pb.set_output(y)
    return pb


def _b_model(size=256, deployed=False, **model_kw):
    cfg = litehandnet_cfg("B", image_size=size)
    cfg.MODEL["ca_dropout"] = 0.0
    cfg.MODEL.update(model_kw)
    m = get_model(cfg)
    return _deploy_without_gpu(m) if deployed else m


def _views(v):
    if isinstance(v, TRef):
        return [v]
    if isinstance(v, TCat):
        return list(v.parts)
    if isinstance(v, (list, tuple)):
        return [t for u in v for t in _views(u)]
    return []


def _rounds(pb):
    """(dilation-1 record, dilation-2 record, gating attention record or None) of an unfused plan, by the rule in the docstring."""
    io = {v.buf for v in (pb.in_ref, pb.out_ref) if v is not None}
    out = []
    for b, rec in enumerate(pb.bufs):
        if b in io:
            continue
        writers = [r for r in pb.recs if r["op"] != TABLE_FILL and any(v.buf == b for v in _views(r.get("out")))]
        if len(writers) != 2 or any(r["op"] != DW for r in writers):
            continue
        d = {r["dil"]: r for r in writers}
        if set(d) != {1, 2}:
            continue
        ok = True
        for dil, r in d.items():
            ok = ok and (r["k"], r["stride"], r["pad"]) == (3, 1, dil) and r["conv"].weight is not None and r.get("bn_repeat", 1) == 1
            ok = ok and r["x"].buf >= 0 and r["x"].C == r["out"].C and r["out"].C in (32, 64, 128) and len(r.get("xs") or [0]) <= 2
        h = d[1]["out"].C
        if not ok or d[2]["out"].C != h or rec.C != 2 * h or (d[1]["out"].coff, d[2]["out"].coff) != (0, h):
            continue
        att = [r for r in pb.recs if r["op"] in (CA_MLP, SE_MLP) and r["y"].buf == b]
        out.append((d[1], d[2], att[0] if att else None))
    return out


def _ops(pb):
    cb, cf, cbw, nf, nb = pb.finalize()
    return [bytes(C.string_at(C.addressof(cf[i]), C.sizeof(cf[i]))) for i in range(nf)], cf, nf


@pytest.mark.parametrize("size", [256, 224])
@pytest.mark.parametrize("deployed", [False, True])
def test_variant_b_rounds_are_fused(size, deployed):
    m = _b_model(size, deployed)
    off = _builder(m, 2, size, False, infer_fuse_msrb=False)
    rounds = _rounds(off)
    assert len(rounds) == 4 and all(a is not None and a["op"] == CA_MLP for _, _, a in rounds)      # 2 MSRBs x 2 rounds
    _, cf_off, nf_off = _ops(off)
    plan.set_infer_fuse_msrb(True)
    on = _builder(m, 2, size, False)
    assert on.infer_fuse_msrb and not on.infer_fuse and not on.infer_fuse_dwpw
    _, cf, nf = _ops(on)
    fused = [r for r in on.recs if r["op"] == MSRB]
    assert len(fused) == 4 == on.n_fused_msrb and on.n_fused == on.n_fused_dwpw == 0
    assert [(id(r["conv"]), id(r["conv2"])) for r in fused] == [(id(a["conv"]), id(b["conv"])) for a, b, _ in rounds]
    assert sum(r["op"] == DW for r in on.recs) == sum(r["op"] == DW for r in off.recs) - 8
    assert not _rounds(on)
    kinds_off, kinds_on = [cf_off[i].kind for i in range(nf_off)], [cf[i].kind for i in range(nf)]
    assert kinds_on.count(AVGPOOL) == kinds_off.count(AVGPOOL) - 4 and kinds_on.count(MSRB) == 4
    assert kinds_on.count(CA_MLP) == kinds_off.count(CA_MLP)
    # the attention MLP behind each fused launch reads the pooled means that launch wrote, and nothing pools in between
    for j in [i for i in range(nf) if cf[i].kind == MSRB]:
        o = cf[j]
        assert o.i[0] == 3 and o.ws[0] >= 0 and o.ws[1] >= 0 and o.ws[1] != o.ws[0]
        assert (cf[j + 1].kind, cf[j + 1].out_buf, cf[j + 1].ws[0]) == (CA_MLP, o.out_buf, o.ws[0])
        half = o.out_C // 2
        assert (o.in_C[0], o.in_C[1], o.out_coff, on.bufs[o.out_buf].C) == (half, half, 0, o.out_C)
        tabs = [(cf[i].out_buf, cf[i].out_coff, cf[i].out_C) for i in (j - 2, j - 1)]      # tables of both halves, just ahead
        assert all(cf[i].kind == (TABLE_FILL if deployed else FINALIZE) for i in (j - 2, j - 1))
        assert tabs == [(o.out_buf, 0, half), (o.out_buf, half, half)]
        if o.i[6] > 1:                                               # second round: out + ca(cat), both coefficients 1
            assert o.in_buf[2] >= 0 and o.i[1] >= 0 and (o.in_C[2], o.i[3]) == (half, half) and (o.f[4], o.f[5]) == (1.0, 1.0)
        else:
            assert o.in_buf[2] == -1 and o.i[1] == -1
    assert sorted(cf[i].i[6] for i in range(nf) if cf[i].kind == MSRB) == [1, 1, 2, 2]
    for (a, b, att), r in zip(rounds, fused):
        assert r["OH"] == 3 and r["pooled"] is not None and r["scratch"] is not None
    pools_of_msrb = {on._abs(r["pooled"]) for r in fused}
    assert not any(cf[i].kind == AVGPOOL and cf[i].ws[0] in pools_of_msrb for i in range(nf))


@pytest.mark.parametrize("ca,oh", [("none", 0), ("se", 1)])
def test_other_attentions(ca, oh):
    m = _b_model(256, msrb_ca=ca)
    off = _builder(m, 2, 256, False, infer_fuse_msrb=False)
    _, cf_off, nf_off = _ops(off)
    on = _builder(m, 2, 256, False, infer_fuse_msrb=True)
    _, cf, nf = _ops(on)
    fused = [r for r in on.recs if r["op"] == MSRB]
    assert len(fused) == 4 == on.n_fused_msrb and [r["OH"] for r in fused] == [oh] * 4
    assert all((r["pooled"] is None) == (oh == 0) and (r["scratch"] is None) == (oh == 0) for r in fused)
    drop = 4 if oh else 0
    assert sum(cf[i].kind == AVGPOOL for i in range(nf)) == sum(cf_off[i].kind == AVGPOOL for i in range(nf_off)) - drop
    for j in [i for i in range(nf) if cf[i].kind == MSRB]:
        assert cf[j].i[0] == oh and (cf[j].ws[0] >= 0) == (oh > 0)
        if oh:
            assert (cf[j + 1].kind, cf[j + 1].ws[0]) == (SE_MLP, cf[j].ws[0])


def test_all_three_switches_on():
    m = _b_model(256)
    both = _builder(m, 2, 256, False, infer_fuse=True, infer_fuse_dwpw=True, infer_fuse_msrb=False)
    both.finalize()
    on = _builder(m, 2, 256, False, infer_fuse=True, infer_fuse_dwpw=True, infer_fuse_msrb=True)
    on.finalize()
    assert on.n_fused_msrb == 4 and (on.n_fused, on.n_fused_dwpw) == (both.n_fused, both.n_fused_dwpw) and on.n_fused_dwpw > 0
    for kind in (PWDW, DWPW):                                        # the other two passes find the pairs they find today
        assert [(id(r["conv"]), id(r["conv2"])) for r in on.recs if r["op"] == kind] == \
               [(id(r["conv"]), id(r["conv2"])) for r in both.recs if r["op"] == kind]
    claimed = [id(c) for r in on.recs if r["op"] in (MSRB, PWDW, DWPW) for c in (r["conv"], r["conv2"])]
    assert len(claimed) == len(set(claimed))                         # no convolution is claimed twice
    left = {id(r["conv"]) for r in on.recs if r["op"] in (DW, PW)}
    assert not left & set(claimed)


def test_switch_off_changes_nothing(monkeypatch):
    for name in ("LHN_INFER_FUSE_MSRB", "LHN_INFER_FUSE_DWPW", "LHN_INFER_FUSE"):
        monkeypatch.delenv(name, raising=False)

    class Old(PlanBuilder):                                          # a builder that never heard of the switch
        def fuse_msrb_round(self):
            return 0
    m = _b_model(256)
    for fuse, dwpw in itertools.product((False, True), repeat=2):
        want = _ops(_builder(m, 2, 256, False, cls=Old, infer_fuse=fuse, infer_fuse_dwpw=dwpw))[0]
        new = _builder(m, 2, 256, False, infer_fuse=fuse, infer_fuse_dwpw=dwpw)
        assert not new.infer_fuse_msrb
        assert _ops(new)[0] == want and new.n_fused_msrb == 0 and not any(r["op"] == MSRB for r in new.recs)
        assert _ops(_builder(m, 2, 256, False, infer_fuse=fuse, infer_fuse_dwpw=dwpw, infer_fuse_msrb=False))[0] == want
        plan.set_infer_fuse_msrb(True)
        assert _ops(_builder(m, 2, 256, False, infer_fuse=fuse, infer_fuse_dwpw=dwpw))[0] != want
        plan.set_infer_fuse_msrb(False)                              # on and then off restores the switch-off op bytes
        assert _ops(_builder(m, 2, 256, False, infer_fuse=fuse, infer_fuse_dwpw=dwpw))[0] == want
        plan.set_infer_fuse_msrb(None)
    monkeypatch.setenv("LHN_INFER_FUSE_MSRB", "1")
    assert plan.infer_fuse_msrb_enabled() and not plan.infer_fuse_enabled() and not plan.infer_fuse_dwpw_enabled()
    pb = _builder(m, 2, 256, False)
    assert pb.infer_fuse_msrb and _ops(pb)[0] != want and pb.n_fused_msrb == 4


def test_training_plans_are_never_rewritten():
    m = _b_model(256)
    plan.set_infer_fuse_msrb(False)
    want = _ops(_builder(m, 2, 256, True))[0]
    plan.set_infer_fuse_msrb(True)
    got = _builder(m, 2, 256, True)
    ops = _ops(got)[0]
    assert got.n_fused_msrb == 0 and not any(r["op"] == MSRB for r in got.recs) and ops == want


def test_unaccepted_width_keeps_its_separate_ops():
    plan.set_infer_fuse_msrb(True)
    pb = _builder(MSRBModule(80, 80, ca_type="ca", p_drop=0.0), 2, 16, False, image=False, cin=80)      # half-width 40
    _, cf, nf = _ops(pb)
    assert pb.n_fused_msrb == 0 and not any(r["op"] == MSRB for r in pb.recs)
    assert sum(r["op"] == DW and r["k"] == 3 for r in pb.recs) == 4 and sum(cf[i].kind == AVGPOOL for i in range(nf)) == 2
    pb = _builder(MSRBModule(64, 64, ca_type="ca", p_drop=0.0), 2, 16, False, image=False, cin=64)      # the same block at half-width 32 is taken
    pb.finalize()
    assert pb.n_fused_msrb == 2 and sum(r["op"] == DW and r["k"] == 3 for r in pb.recs) == 0


def test_symbols_are_declared_listed_and_exported():
    with open(os.path.join(ROOT, "include", "lhn.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+lhn_msrb_round_fwd\s*\(", header) and re.search(r"\bint64_t\s+lhn_msrb_round_scratch_bytes\s*\(", header)
    so = C.CDLL(_lib.LIB_PATH)
    for name in ("lhn_msrb_round_fwd", "lhn_msrb_round_scratch_bytes"):
        assert name in _lib.SYMBOLS and hasattr(so, name)
    L = _lib.lib()
    assert len(L.lhn_msrb_round_fwd.argtypes) == 11 and L.lhn_msrb_round_scratch_bytes.restype is C.c_int64
    assert L.lhn_msrb_round_scratch_bytes(2, 64, 64, 128) == 2 * 8 * 2 * 9 * 128 * 4      # host-only: no device needed
    assert L.lhn_msrb_round_scratch_bytes(2, 64, 64, 80) == 0
    assert L.lhn_version() == 3
