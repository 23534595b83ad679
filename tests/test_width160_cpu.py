"""CPU: `mynet` at input_channel = 160 (the reference's config/mynet/w160 files) in the plan compiler and the oracle -- no GPU, no
kernel launch.  None of the inference rewrites is built for this width (the BottleNeck pass matches variant A's blocks, the stem
tail is 32 -> 128, bf16x3 takes 32 / 64 / 128 channels), so the inference plan with every switch on is the plan with every switch
off, op for op and byte for byte; and the oracle reproduces the real reference's fixture (tests/golden/make_golden_w160.py)."""
import ctypes as C

import pytest

import plan_digest
from litehandnet_amd import get_model, plan
from litehandnet_amd.config import litehandnet_cfg
from litehandnet_amd.plan import BNECK, DWPW, KXK, MSRB, PWDW, STEMTAIL, PlanBuilder
from oracle import torch_ref
from test_oracle_golden import _run_case

WIDTH = 160
SWITCHES = ("LHN_INFER_BF16X3", "LHN_INFER_FUSE_BNECK", "LHN_INFER_FUSE_MSRB", "LHN_INFER_FUSE_DWPW", "LHN_INFER_FUSE", "LHN_INFER_FUSE_STEM",
            "LHN_INFER_FUSE_CCW")
ALL_ON = dict(infer_fuse=True, infer_fuse_dwpw=True, infer_fuse_msrb=True, infer_fuse_bneck=True, infer_bf16x3=True, infer_fuse_stem=True,
              infer_fuse_ccw=True)
ALL_OFF = {k: False for k in ALL_ON}


@pytest.fixture(autouse=True)
def _switches_back(monkeypatch):
    for name in SWITCHES + tuple(plan_digest.SWITCHES):
        monkeypatch.delenv(name, raising=False)
    yield


def _builder(m, size, **kw):
    tensors = list(m.state_dict(keep_vars=True).values())
    pb = PlanBuilder(2, {id(t): j for j, t in enumerate(tensors)}, image_hw=(size, size), with_backward=False, p_drop=0.0, **kw)
    y = m.emit(pb, pb.image())
    if getattr(y, "buf", None) != -2:
        pb.set_output(y)
    return pb


def _ops(pb):
    cb, cf, _, nf, _ = pb.finalize()
    return [bytes(C.string_at(C.addressof(cf[i]), C.sizeof(cf[i]))) for i in range(nf)], bytes(C.string_at(C.addressof(cb), C.sizeof(cb)))


@pytest.mark.parametrize("size", [64, 256])
def test_inference_switches_rewrite_nothing_at_160(size):
    cfg = litehandnet_cfg("M", channels=WIDTH, image_size=size)
    cfg.MODEL["ca_dropout"] = 0.0
    m = get_model(cfg)
    off, on = _builder(m, size, **ALL_OFF), _builder(m, size, **ALL_ON)
    assert _ops(on) == _ops(off)
    assert (on.n_fused, on.n_fused_dwpw, on.n_fused_msrb, on.n_fused_bneck, on.n_bf16x3) == (0, 0, 0, 0, 0)
    for _, _, _, counter, _ in plan.INFER_SWITCHES:
        assert getattr(on, counter) == 0, counter
    assert not any(r["op"] in (PWDW, DWPW, MSRB, BNECK, STEMTAIL) or r.get("bf16x3") for r in on.recs)
    # the dense 3x3 of the model: 160 -> 160 (two per BasicBlock) and 40 -> 40 (one per BottleNeck, one in the stem), nothing else
    kxk = [(r["x"].C, r["out"].C) for r in on.recs if r["op"] == KXK]
    from litehandnet_amd import pose_hg_ms_att as pm
    nbb = sum(isinstance(x, pm.BasicBlock) for x in m.modules())
    nbn = sum(isinstance(x, pm.BottleNeck) for x in m.modules())
    assert sorted(set(kxk)) == [(40, 40), (160, 160)]
    assert kxk.count((160, 160)) == 2 * nbb and kxk.count((40, 40)) == nbn + 1
    assert not any(plan.bf16x3_eligible(ci, co, 1) for ci, co in kxk)


def test_oracle_reproduces_the_reference_at_160(golden_dir):
    """`mynet` at width 160: the oracle against the fixture the real reference wrote (fp32 and float64); 3,490,101 parameters."""
    _run_case(golden_dir, "M160_64", "M", channels=WIDTH)
    m = torch_ref.get_model(litehandnet_cfg("M", channels=WIDTH))
    assert sum(p.numel() for p in m.parameters()) == 3490101
