"""GPU: Lite-HRNet with the ConditionalChannelWeighting inference switch on (plan.set_infer_fuse_ccw): every block runs as four
grouped launches (lhn_ccw_pool_fwd, lhn_ccw_gate_fwd, lhn_ccw_dw_fwd, lhn_ccw_shuffle_fwd).  Criteria of tests/test_infer_fuse_gpu.py:
the arbiter is the float64 oracle, the yardstick is the UNFUSED forward of the same process on the same inputs; the fused forward
may be at most 3x as far from float64 (floor 1e-4 of the heat maps' peak), and its argmax coordinates equal the unfused ones except
at near-ties of the float64 map."""
import ctypes as C

import pytest
import torch

from litehandnet_amd import get_model, plan
from litehandnet_amd.config import litehandnet_cfg
from litehandnet_amd.plan import CCW_DW, CCW_GATE, CCW_POOL, CCW_SHUFFLE, DW, FINALIZE, SE_MLP
from oracle import synth, torch_ref
from test_infer_fuse_gpu import _compare, _pair

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _switches_back():
    yield
    plan.set_infer_fuse_ccw(None)


@pytest.fixture
def all_classes(monkeypatch):
    """The pass over blocks of 2, 3 and 4 branches (the default leaves the two-branch class out: profiles/infer_fuse_ccw.md)."""
    monkeypatch.setattr(plan.PlanBuilder, "FUSE_CCW_BRANCHES", (2, 3, 4))


def _fwd(m, x, ccw):
    """Forward with the switch as given (the other six off); returns (heat maps, the plan)."""
    plan.set_infer_fuse_ccw(ccw)
    with torch.no_grad():
        y = m(x).clone()
    p = [p for k, p in m.__dict__["_engine"].plans.items()
         if k[0] == tuple(x.shape) and k[1] is False and k[-7] == bool(ccw) and not any(k[-6:])]
    assert len(p) == 1
    return y, p[0]


def _pair30(size, seed):
    """_pair for Lite-HRNet-30."""
    cfg = litehandnet_cfg("L", image_size=size, depth=30)
    ref = torch_ref.get_model(cfg, p_drop=0.0)
    sd = synth.synth_state_dict(ref, seed)
    ref.load_state_dict(sd)
    m = get_model(cfg)
    m.load_state_dict(sd)
    return m, ref.double().eval()


@pytest.mark.parametrize("depth,size,n_blocks", [(18, 64, 20), (18, 128, 20), (30, 64, 28)])
def test_litehrnet_eval(dev, depth, size, n_blocks, all_classes):
    m, ref = _pair("L", size, 31) if depth == 18 else _pair30(size, 31)
    m.to(dev).eval()
    x = synth.synth_images(2, size, 5)
    with torch.no_grad():
        y64 = ref(x.double())
    xg = x.to(dev)
    y_u, p_u = _fwd(m, xg, False)
    y_f, p_f = _fwd(m, xg, True)
    assert p_u.pb.n_fused_ccw == 0 and p_f.pb.n_fused_ccw == n_blocks
    kinds = [r["op"] for r in p_f.pb.recs]
    assert all(kinds.count(k) == n_blocks for k in (CCW_POOL, CCW_GATE, CCW_DW, CCW_SHUFFLE)) and SE_MLP not in kinds
    assert not any(r["op"] == DW and r["k"] == 3 and r["stride"] == 1 and r["conv"].bias is not None for r in p_f.pb.recs)
    _compare(f"ccw/L{depth}_{size}_eval", y_f, y_u, y64)
    with torch.no_grad():                          # second run of a plan: tables reused, same bits
        assert torch.equal(m(xg), y_f)
    assert torch.equal(_fwd(m, xg, True)[0], y_f)
    assert torch.equal(_fwd(m, xg, False)[0], y_u)


def test_default_classes_at_64(dev):
    """The default pass (blocks of 3 and 4 branches; the two-branch blocks keep their separate launches) under the same criteria."""
    m, ref = _pair("L", 64, 37)
    m.to(dev).eval()
    x = synth.synth_images(2, 64, 6)
    with torch.no_grad():
        y64 = ref(x.double())
    xg = x.to(dev)
    y_u, _ = _fwd(m, xg, False)
    y_f, p_f = _fwd(m, xg, True)
    assert p_f.pb.n_fused_ccw == 14 and sorted({len(r["x2"]) for r in p_f.pb.recs if r["op"] == CCW_POOL}) == [3, 4]
    assert sum(r["op"] == SE_MLP for r in p_f.pb.recs) == 12
    _compare("ccw/L18_64_eval_default", y_f, y_u, y64)
    assert torch.equal(_fwd(m, xg, True)[0], y_f)


def test_tables_follow_the_parameters(dev, all_classes):
    """The table cache covers the tables the grouped launches read: after a depthwise BatchNorm's running variance or a
    SpatialWeighting bias changes, the next fused eval forward equals one from a freshly built plan."""
    m, _ = _pair("L", 64, 43)
    m.to(dev).eval()
    x = synth.synth_images(2, 64, 7).to(dev)
    y1, p = _fwd(m, x, True)
    assert torch.equal(_fwd(m, x, True)[0], y1) and p._table_sig is not None

    def fresh():
        m.__dict__.pop("_engine", None)
        return _fwd(m, x, True)[0]
    dw = next(r for r in p.pb.recs if r["op"] == CCW_DW)
    bn = next(r["bn"] for r in p.pb.recs if r["op"] == FINALIZE and r["out"].buf == dw["ys"][0].buf)
    with torch.no_grad():
        bn.running_var.mul_(2.0)
    y2, _ = _fwd(m, x, True)
    assert not torch.equal(y2, y1) and torch.equal(y2, fresh())
    sw = m.stage0[0].layers[0].spatial_weighting[0]
    with torch.no_grad():
        sw.conv2[0].bias.add_(0.5)
    y3, _ = _fwd(m, x, True)
    assert not torch.equal(y3, y2) and torch.equal(y3, fresh())
    crw = m.stage2[0].layers[1].cross_resolution_weighting
    with torch.no_grad():
        crw.conv1[0].bias.add_(0.5)                # a bias in front of a BatchNorm: folded into the table the gate launch reads
    y4, _ = _fwd(m, x, True)
    assert not torch.equal(y4, y3) and torch.equal(y4, fresh())


def test_train_mode_and_backward_are_untouched(dev):
    m, _ = _pair("L", 64, 47)
    m.to(dev)
    x = synth.synth_images(2, 64, 9).to(dev)
    state = {k: v.clone() for k, v in m.state_dict().items()}

    def run(ccw, grad):
        m.__dict__.pop("_engine", None)
        m.load_state_dict(state)
        m.train()
        plan.set_infer_fuse_ccw(ccw)
        if grad:
            y = m(x)
            y.square().mean().backward()
            out = [y.detach().clone()] + [p.grad.clone() for p in m.parameters() if p.grad is not None]
            m.zero_grad(set_to_none=True)
        else:
            with torch.no_grad():
                out = [m(x).clone()]
        plans = list(m.__dict__["_engine"].plans.values())
        assert len(plans) == 1 and plans[0].pb.n_fused_ccw == 0 and not plans[0].pb.infer_fuse_ccw
        ops = [b"" if a is None else bytes(C.string_at(C.addressof(a), C.sizeof(a))) for a in plans[0]._keep]
        return out, ops
    for grad in (False, True):
        (a, ops_a), (b, ops_b) = run(False, grad), run(True, grad)
        assert ops_a == ops_b, "the switch changed a plan that runs train-mode BatchNorm"
        assert len(a) == len(b) and (len(ops_a[2]) > 0) == grad
        # the same launches on the same inputs: equal up to the order of the statistics' atomic adds
        assert float((a[0] - b[0]).abs().max()) <= 1e-5 * float(a[0].abs().max())
