"""GPU: whole models with the depthwise -> 1x1 inference fusion switch on (plan.set_infer_fuse_dwpw): the eligible DWConv pairs run
as one launch each (lhn_conv_dw3_pw_fwd).  Criteria of tests/test_infer_fuse_gpu.py: the arbiter is the float64 oracle, the
yardstick is the UNFUSED forward of the same process on the same inputs; the fused forward may be at most 3x as far from float64
(floor 1e-4 of the heat maps' peak), and its argmax coordinates equal the unfused ones except at near-ties of the float64 map."""
import os

import numpy as np
import pytest
import torch

from litehandnet_amd import get_model, plan
from litehandnet_amd.config import litehandnet_cfg
from litehandnet_amd.plan import DWPW, FINALIZE, PWDW
from oracle import synth
from test_infer_fuse_gpu import _compare, _pair
from test_model_gpu import FWD_TOL, _rel

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _switches_back():
    yield
    plan.set_infer_fuse(None)
    plan.set_infer_fuse_dwpw(None)


def _fwd(m, x, dwpw, fuse=False):
    plan.set_infer_fuse(fuse)
    plan.set_infer_fuse_dwpw(dwpw)
    with torch.no_grad():
        y = m(x).clone()
    p = [p for k, p in m.__dict__["_engine"].plans.items() if k[0] == tuple(x.shape) and k[-1] == bool(fuse) and k[-2] == bool(dwpw)]
    assert len(p) == 1
    return y, p[0]


@pytest.mark.parametrize("size", [256, 224])
def test_variant_a_eval_and_deployed(dev, size):
    m, ref = _pair("A", size, 23)
    m.to(dev).eval()
    x = synth.synth_images(2, size, 5)
    with torch.no_grad():
        y64 = ref(x.double())
        y64 = y64[-1] if isinstance(y64, (tuple, list)) else y64
    xg = x.to(dev)
    y_u, p_u = _fwd(m, xg, False)
    y_f, p_f = _fwd(m, xg, True)
    y_b, p_b = _fwd(m, xg, True, True)
    assert p_u.pb.n_fused_dwpw == 0 and p_f.pb.n_fused_dwpw == 16 and p_f.pb.n_fused == 0
    assert p_b.pb.n_fused_dwpw == 16 and sum(r["op"] == PWDW for r in p_b.pb.recs) == p_b.pb.n_fused
    _compare(f"dwpw/A_{size}_eval", y_f, y_u, y64)
    _compare(f"dwpw/A_{size}_eval_both", y_b, y_u, y64)
    with torch.no_grad():                          # second run of a plan: tables reused, same bits
        assert torch.equal(m(xg), y_b)
    m.deploy_model()
    d_u, q_u = _fwd(m, xg, False)
    d_f, q_f = _fwd(m, xg, True)
    assert torch.equal(_fwd(m, xg, True)[0], d_f)
    d_b, q_b = _fwd(m, xg, True, True)
    assert torch.equal(_fwd(m, xg, True, True)[0], d_b)
    assert q_u.pb.n_fused_dwpw == 0 and q_f.pb.n_fused_dwpw == 16 and q_b.pb.n_fused_dwpw == 16
    for q in (q_f, q_b):
        assert not any(r["op"] == FINALIZE for r in q.pb.recs)
    _compare(f"dwpw/A_{size}_deployed", d_f, d_u, y64)
    _compare(f"dwpw/A_{size}_deployed_both", d_b, d_u, y64)


def test_variant_a_deployed_golden(dev, golden_dir):
    """The fused deployed forward against the reference's recorded heat maps, at the tolerance test_deploy_model_golden holds the
    unfused forward to.  The 64 x 64 image takes the kernel to 16 x 16 and 8 x 8 maps."""
    g = np.load(os.path.join(golden_dir, "model_A_64_deploy.npz"))
    m = get_model(litehandnet_cfg("A"))
    m.load_state_dict(synth.synth_state_dict(m, int(g["weights_seed"])))
    m.to(dev).eval()
    x = synth.synth_images(2, 64, int(g["seed"])).to(dev)
    y_eval, p = _fwd(m, x, True)
    assert p.pb.n_fused_dwpw == 16
    assert {r["x"].H for r in p.pb.recs if r["op"] == DWPW} == {16, 8}
    m.deploy_model()
    y, q = _fwd(m, x, True)
    assert q.pb.n_fused_dwpw == 16
    ref = g["heatmap"]
    assert np.abs(y.cpu().numpy() - ref).max() <= FWD_TOL * np.abs(ref).max()
    assert _rel(y, y_eval) < 1e-4


def test_tables_follow_the_parameters(dev):
    """The table cache covers t_table: after a parameter of a fused pair changes, or a train-mode run moves the running
    statistics, the next fused eval forward equals one from a freshly built plan."""
    m, _ = _pair("A", 64, 43)
    m.to(dev).eval()
    x = synth.synth_images(2, 64, 7).to(dev)
    y1, p = _fwd(m, x, True)
    y1b, _ = _fwd(m, x, True)
    assert torch.equal(y1, y1b) and p._table_sig is not None

    def fresh():
        m.__dict__.pop("_engine", None)
        return _fwd(m, x, True)[0]
    fin = [r for r in p.pb.recs if r["op"] == FINALIZE]
    mids = {r["mid"].buf for r in p.pb.recs if r["op"] == DWPW}
    bn1 = next(r["bn"] for r in fin if r["out"].buf in mids)       # BatchNorm between the two convolutions of a fused pair
    with torch.no_grad():
        bn1.bias.add_(0.5)
        bn1.running_var.mul_(2.0)
    y2, _ = _fwd(m, x, True)
    assert not torch.equal(y2, y1)
    assert torch.equal(y2, fresh())
    m.train()
    with torch.no_grad():                          # train-mode BatchNorm under no_grad: runs the unfused plan, moves the statistics
        m(synth.synth_images(4, 64, 8).to(dev))
    m.eval()
    y3, _ = _fwd(m, x, True)
    assert not torch.equal(y3, y2)
    assert torch.equal(y3, fresh())
    plan.invalidate_tables()
    assert torch.equal(_fwd(m, x, True)[0], y3)


@pytest.mark.parametrize("variant", ["B", "M"])
def test_other_variants_eval(dev, variant):
    m, ref = _pair(variant, 256, 31)
    m.to(dev).eval()
    x = synth.synth_images(1, 256, 6)
    with torch.no_grad():
        y64 = ref(x.double())
        y64 = y64[-1] if isinstance(y64, (tuple, list)) else y64
    xg = x.to(dev)
    y_u, _ = _fwd(m, xg, False)
    y_f, p_f = _fwd(m, xg, True)
    fused = [r for r in p_f.pb.recs if r["op"] == DWPW]
    assert len(fused) == p_f.pb.n_fused_dwpw                       # whatever number the rule finds there
    print(f"{variant}: {len(fused)} depthwise -> 1x1 pairs")
    _compare(f"dwpw/{variant}_256_eval", y_f, y_u, y64)
