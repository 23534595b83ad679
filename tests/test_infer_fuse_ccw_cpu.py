"""CPU: the ConditionalChannelWeighting inference pass of the plan compiler (PlanBuilder.fuse_ccw, switched by LHN_INFER_FUSE_CCW=1 or
plan.set_infer_fuse_ccw) -- no GPU, no kernel launch.  A block, as this file finds it in the switch-off plan independently of the
pass: a whole buffer that only adaptive average pools write (2..4 of them, side by side, to the buffer's own map size) and only
one 1x1 convolution reads; the records between that 1x1 and the channel shuffles are then counted, not matched: two 1x1, two
sigmoid(relu(.)) combines, and per pool one product, one 3x3 depthwise convolution, one SE_MLP of mode 1 and one SHUFFLE."""
import ctypes as C
import json
import os
import re

import pytest

import plan_digest
from litehandnet_amd import _lib, engine, get_model, plan
from litehandnet_amd.config import litehandnet_cfg
from litehandnet_amd.plan import (AVGPOOL, CCW_ARG, CCW_DW, CCW_GATE, CCW_POOL, CCW_SHUFFLE, DW, EW, EW_MUL, FINALIZE, PW, SE_MLP, SHUFFLE,
                                  SLOPE_RELU_SIGMOID, PlanBuilder, TCat, TRef)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CCW = (CCW_POOL, CCW_GATE, CCW_DW, CCW_SHUFFLE)


@pytest.fixture(autouse=True)
def _switches_back():
    plan.set_infer_fuse_ccw(None)
    yield
    plan.set_infer_fuse_ccw(None)


@pytest.fixture
def all_classes(monkeypatch):
    """The pass over blocks of 2, 3 and 4 branches.  The default leaves the two-branch class out (it did not pass the keep-or-drop rule
    of profiles/infer_fuse_ccw.md on its own); the pass itself and the entry points take all three."""
    monkeypatch.setattr(PlanBuilder, "FUSE_CCW_BRANCHES", (2, 3, 4))


_MODELS = {}


def _model(variant="L", depth=18):
    if (variant, depth) not in _MODELS:
        kw = dict(depth=depth) if variant == "L" else {}
        cfg = litehandnet_cfg(variant, **kw)
        cfg.MODEL["ca_dropout"] = 0.0
        _MODELS[(variant, depth)] = get_model(cfg).eval()
    return _MODELS[(variant, depth)]


def _builder(m, size, backward=False, cls=PlanBuilder, **kw):
    tensors = list(m.state_dict(keep_vars=True).values())
    pb = cls(2, {id(t): j for j, t in enumerate(tensors)}, image_hw=(size, size), with_backward=backward, p_drop=0.0, **kw)
    y = m.emit(pb, pb.image())
    if getattr(y, "buf", None) != -2:
        pb.set_output(y)
    return pb


def _ops(pb):
    cb, cf, cbw, nf, nb = pb.finalize()
    return [bytes(C.string_at(C.addressof(cf[i]), C.sizeof(cf[i]))) for i in range(nf)], cf, nf


def _views(v):
    if isinstance(v, TRef):
        return [v]
    if isinstance(v, TCat):
        return list(v.parts)
    if isinstance(v, (list, tuple)):
        return [t for u in v for t in _views(u)]
    return []


def _sig(r):
    """What a record is, apart from its identity: its kind, its modules and every view it holds."""
    views = tuple((k, tuple((v.buf, v.coff, v.C, v.H, v.W) for v in _views(u))) for k, u in sorted(r.items()) if _views(u))
    return (r["op"], id(r.get("conv")), id(r.get("bn")), id(r.get("se")), r.get("slope"), r.get("mode"), views)


def _blocks(pb):
    """[(the records of a block, branches, integer ratios?)] of an unfused plan, by the rule in the docstring."""
    out = []
    for b, rec in enumerate(pb.bufs):
        writers = [r for r in pb.recs if any(v.buf == b for v in _views(r.get("out")))]
        readers = [r for r in pb.recs if any(v.buf == b for k, u in r.items() if k != "out" for v in _views(u))]
        if not 2 <= len(writers) <= 4 or any(r["op"] != AVGPOOL or (r["OH"], r["OW"]) != (rec.H, rec.W) for r in writers):
            continue
        if len(readers) != 1 or readers[0]["op"] != PW or sum(r["out"].C for r in writers) != rec.C:
            continue
        first = pb.recs.index(readers[0])
        last = first
        n_sh = 0
        while n_sh < len(writers):                      # the block ends with its last channel shuffle
            last += 1
            n_sh += pb.recs[last]["op"] == SHUFFLE
        inner = pb.recs[first:last + 1]
        B = len(writers)
        count = lambda f: sum(bool(f(r)) for r in inner)
        assert count(lambda r: r["op"] == PW) == 2 and count(lambda r: r["op"] == EW and r["slope"] == SLOPE_RELU_SIGMOID) == 2
        assert count(lambda r: r["op"] == EW and r.get("mode") == EW_MUL) == B == count(lambda r: r["op"] == DW and r["k"] == 3)
        assert count(lambda r: r["op"] == SE_MLP and r["mode"] == 1) == B and len(inner) == 4 + 4 * B
        integer = all(r["x"].H % rec.H == 0 and r["x"].W % rec.W == 0 for r in writers)
        out.append((writers + inner, B, integer))
    return out


@pytest.mark.parametrize("size", [256, 224, 64])
@pytest.mark.parametrize("depth,n_blocks,n_rec", [(18, 20, 602), (30, 28, 826)])
def test_litehrnet_blocks_are_rewritten(depth, n_blocks, n_rec, size, all_classes):
    m = _model("L", depth)
    off = _builder(m, size)
    blocks = _blocks(off)
    assert len(blocks) == n_blocks and len(off.recs) == n_rec and all(integer for _, _, integer in blocks)
    if depth == 18:
        assert sorted(B for _, B, _ in blocks) == [2] * 6 + [3] * 8 + [4] * 6
    _, cf_off, nf_off = _ops(off)
    plan.set_infer_fuse_ccw(True)
    on = _builder(m, size, infer_fuse_ccw=None)
    assert on.infer_fuse_ccw and not (on.infer_fuse or on.infer_fuse_dwpw or on.infer_fuse_msrb or on.infer_fuse_bneck or on.infer_fuse_stem)
    _, cf, nf = _ops(on)
    assert on.n_fused_ccw == n_blocks and not _blocks(on)
    assert on.n_fused == on.n_fused_dwpw == on.n_fused_msrb == on.n_fused_bneck == on.n_fused_stem == on.n_bf16x3 == 0
    # none of the replaced records is left, every other record is unchanged and in the same order
    gone = {id(r) for recs, _, _ in blocks for r in recs}
    assert len(gone) == sum(4 + 5 * B for _, B, _ in blocks)
    kept = [_sig(r) for r in on.recs if r["op"] not in CCW + (FINALIZE,)]
    assert kept == [_sig(r) for r in off.recs if id(r) not in gone] and len(kept) == len(off.recs) - len(gone)
    assert not {_sig(r) for r in off.recs if id(r) in gone} & set(kept)
    # four launch records per block, in order, behind the 2 + B tables they read
    kinds = [r["op"] for r in on.recs]
    at = [j for j, k in enumerate(kinds) if k == CCW_POOL]
    assert len(at) == n_blocks
    for j, (_, B, _) in zip(at, blocks):
        assert tuple(kinds[j:j + 4]) == CCW and kinds[j - 2 - B:j] == [FINALIZE] * (2 + B)
        pool, gate, dw, sh = on.recs[j:j + 4]
        assert len(pool["x2"]) == B and dw["scratch"] is sh["scratch"] and dw["g"] == gate["out"] and gate["x"] == pool["out"]
        tabs = [(r["out"].buf, r["out"].C, r["bias"] is not None) for r in on.recs[j - 2 - B:j]]
        assert tabs[:2] == [(gate["mids"][0].buf, gate["mid"], True), (gate["mids"][1].buf, pool["out"].C, True)]
        assert tabs[2:] == [(y.buf, y.C, True) for y in dw["ys"]]
    # launches of a steady-state forward: 16 / 22 / 28 per block become 4
    launches = lambda c, n: sum(c[i].kind not in (plan.TABLE_FILL, FINALIZE, plan.MEMSET, CCW_ARG) for i in range(n))
    assert launches(cf_off, nf_off) - launches(cf, nf) == sum(4 + 6 * B - 4 for _, B, _ in blocks)
    if depth == 18:
        assert (launches(cf_off, nf_off), launches(cf, nf)) == (662, 302)
    # every grouped launch stands behind one CCW_ARG op per branch
    for i in range(nf):
        if cf[i].kind in (CCW_POOL, CCW_DW, CCW_SHUFFLE):
            B = cf[i].i[0]
            assert 2 <= B <= 4 and all(cf[i - k].kind == CCW_ARG for k in range(1, B + 1)) and cf[i - B - 1].kind != CCW_ARG
            for k in range(1, B + 1):
                a = cf[i - k]
                assert a.in_C[0] == a.in_C[1] == a.in_C[2] and a.out_C == 2 * a.in_C[0] and a.i[0] == a.in_C[0] // 4 and min(a.p[:5]) >= 0
        if cf[i].kind in (CCW_DW, CCW_SHUFFLE):
            assert cf[i].ws[0] >= 0


def test_default_classes():
    """By default the blocks of 3 and 4 branches are rewritten and the six two-branch blocks of stage 2 stay as they are."""
    assert PlanBuilder.FUSE_CCW_BRANCHES == (3, 4)
    for depth, n_all, n_default in ((18, 20, 14), (30, 28, 22)):
        m = _model("L", depth)
        off = _builder(m, 64)
        blocks = _blocks(off)
        assert len(blocks) == n_all and sum(B > 2 for _, B, _ in blocks) == n_default
        on = _builder(m, 64, infer_fuse_ccw=True)
        on.finalize()
        left = _blocks(on)
        assert on.n_fused_ccw == n_default and [B for _, B, _ in left] == [2] * 6
        stay = [_sig(r) for recs, B, _ in blocks if B == 2 for r in recs]
        assert set(stay) <= {_sig(r) for r in on.recs}
        assert sorted(len(r["x2"]) for r in on.recs if r["op"] == CCW_POOL) == sorted(B for _, B, _ in blocks if B > 2)


def test_plans_with_a_backward_and_other_families_are_untouched(all_classes):
    m = _model("L")
    plan.set_infer_fuse_ccw(False)
    want = _ops(_builder(m, 64, backward=True, infer_fuse_ccw=None))[0]
    plan.set_infer_fuse_ccw(True)
    got = _builder(m, 64, backward=True, infer_fuse_ccw=None)
    assert _ops(got)[0] == want and got.n_fused_ccw == 0 and not any(r["op"] in CCW for r in got.recs)
    for v in "ABMH":
        mv = _model(v)
        off, on = _builder(mv, 64), _builder(mv, 64, infer_fuse_ccw=True)
        assert _ops(on)[0] == _ops(off)[0] and on.n_fused_ccw == 0


@pytest.mark.parametrize("size,n_fused", [(100, 0), (80, 14), (96, 20)])
def test_only_blocks_with_integer_ratios_are_rewritten(size, n_fused, all_classes):
    """100: maps of 25 / 13 / 7 / 4, no block has integer ratios; 80: 20 / 10 / 5 / 3, the four-branch blocks stay; 96: 24 / 12 / 6 / 3."""
    m = _model("L")
    off = _builder(m, size)
    blocks = _blocks(off)
    assert len(blocks) == 20 and sum(integer for _, _, integer in blocks) == n_fused
    on = _builder(m, size, infer_fuse_ccw=True)
    on.finalize()
    assert on.n_fused_ccw == n_fused
    left = _blocks(on)
    assert len(left) == 20 - n_fused and not any(integer for _, _, integer in left)
    stay = {_sig(r) for recs, _, integer in blocks if not integer for r in recs}
    assert stay <= {_sig(r) for r in on.recs}


def test_switch_off_changes_nothing(monkeypatch, all_classes):
    for name in plan_digest.INFER_ENV + ("LHN_INFER_FUSE_CCW",):
        monkeypatch.delenv(name, raising=False)
    with open(os.path.join(ROOT, "tests", "plan_digests_infer.json")) as f:
        pinned = json.load(f)["configs"]["L_eval_all"]
    assert plan_digest.infer_digest(plan_digest.build("L_eval_all")) == pinned       # the parent's digest, switch off

    class Old(PlanBuilder):                                          # a builder that never heard of the switch
        def fuse_ccw(self):
            return 0
    m = _model("L")
    want = _ops(_builder(m, 64, cls=Old))[0]
    new = _builder(m, 64)
    assert not new.infer_fuse_ccw and not plan.infer_fuse_ccw_enabled()
    assert _ops(new)[0] == want and new.n_fused_ccw == 0
    plan.set_infer_fuse_ccw(True)
    assert _ops(_builder(m, 64, infer_fuse_ccw=None))[0] != want
    assert _ops(_builder(m, 64))[0] == want                          # the keyword's default is False, whatever the process switch says
    plan.set_infer_fuse_ccw(None)
    monkeypatch.setenv("LHN_INFER_FUSE_CCW", "1")
    assert plan.infer_fuse_ccw_enabled() and not any(f() for f in (plan.infer_fuse_enabled, plan.infer_fuse_dwpw_enabled, plan.infer_fuse_msrb_enabled,
                                                                   plan.infer_fuse_bneck_enabled, plan.infer_fuse_stem_enabled, plan.infer_bf16x3_enabled))
    pb = _builder(m, 64, infer_fuse_ccw=None)
    assert _ops(pb)[0] != want and pb.n_fused_ccw == 20
    assert plan.INFER_SWITCHES[-1][:4] == ("infer_fuse_ccw", "LHN_INFER_FUSE_CCW", "fuse_ccw", "n_fused_ccw") and len(plan.INFER_SWITCHES) == 7


def test_with_the_other_six_switches_on(all_classes):
    """The patterns are disjoint: with all seven on, Lite-HRNet's plan has the blocks of this pass and nothing of the others."""
    m = _model("L")
    six = {k: True for k in plan_digest.INFER_KW}
    base, on = _builder(m, 64, **six), _builder(m, 64, infer_fuse_ccw=True, **six)
    base.finalize()
    on.finalize()
    counters = lambda pb: [getattr(pb, k) for k in plan_digest.INFER_COUNTERS]
    assert on.n_fused_ccw == 20 and counters(on) == counters(base)


def test_symbols_are_declared_listed_and_exported():
    with open(os.path.join(ROOT, "include", "lhn.h")) as f:
        header = f.read()
    so = C.CDLL(_lib.LIB_PATH)
    for name in ("lhn_ccw_pool_fwd", "lhn_ccw_gate_fwd", "lhn_ccw_dw_fwd", "lhn_ccw_shuffle_fwd"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header) and name in _lib.SYMBOLS and hasattr(so, name)
    assert re.search(r"\bint64_t\s+lhn_ccw_scratch_bytes\s*\(", header) and "lhn_ccw_scratch_bytes" in _lib.SYMBOLS and hasattr(so, "lhn_ccw_scratch_bytes")
    L = _lib.lib()
    assert L.lhn_ccw_scratch_bytes.restype is C.c_int64 and len(L.lhn_ccw_gate_fwd.argtypes) == 12
    arr = lambda *v: (C.c_int * len(v))(*v)
    # host-only: no device needed.  Tiles of (256 / (C / 4)) * 2 pixels: 16 x 16 x 20 -> 3 tiles, 8 x 8 x 40 -> 2
    assert L.lhn_ccw_scratch_bytes(2, 2, arr(16, 8), arr(16, 8), arr(20, 40)) == 2 * (3 * 20 + 2 * 40) * 4
    assert L.lhn_ccw_scratch_bytes(2, 2, arr(12, 8), arr(12, 8), arr(20, 40)) == 0          # 12 is no multiple of 8
    assert L.lhn_ccw_scratch_bytes(2, 2, arr(8, 16), arr(8, 16), arr(20, 40)) == 0          # smallest map first
    assert L.lhn_ccw_scratch_bytes(2, 2, arr(16, 8), arr(16, 8), arr(164, 40)) == 0
    assert L.lhn_ccw_scratch_bytes(2, 1, arr(16), arr(16), arr(20)) == 0 and L.lhn_ccw_scratch_bytes(2, 5, arr(*[8] * 5), arr(*[8] * 5), arr(*[20] * 5)) == 0


def test_cache_key_keeps_its_tail():
    """Engine.plan_for's key: the new flag is inserted in front of fuse_stem, so k[-1] .. k[-6] mean what they meant and k[-7] is the
    new flag.  Read from the source: building a plan needs the GPU (tests/test_infer_fuse_ccw_gpu.py looks at real keys)."""
    import inspect
    src = inspect.getsource(engine.Engine.plan_for)
    base = [t.strip() for t in re.search(r"key = \(([^\n]*)\)\n", src).group(1).split(",")]
    assert base[4:] == ["fuse_stem", "bf16x3", "fuse_bneck", "fuse_msrb", "fuse_dwpw", "fuse"] and len(base) == 10
    assert "key = key[:4] + (fuse_ccw,) + key[4:]" in src and "infer_fuse_ccw=fuse_ccw" in src
    assert "infer_fuse_ccw_enabled() and not with_backward and (deployed or not self.module.training)" in src
