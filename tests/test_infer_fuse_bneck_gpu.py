"""GPU: whole models with the BottleNeck inference fusion on (plan.set_infer_fuse_bneck): every BottleNeck -- 1x1, 3x3, 1x1, residual
sum, activation -- runs as one launch (lhn_bottleneck_fwd).  The arbiter is the float64 oracle; the yardstick is the UNFUSED forward of
the same process on the same inputs, with the criterion of tests/test_infer_fuse_gpu.py (_compare): at most 3x the unfused distance
from float64, floor 1e-4 of the heat maps' peak, argmax equal except at near-ties."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from litehandnet_amd import get_model, plan
from litehandnet_amd.config import litehandnet_cfg
from litehandnet_amd.plan import BNECK, FINALIZE
from oracle import synth, torch_ref
from test_infer_fuse_gpu import _compare, _pair
from test_model_gpu import FWD_TOL, _rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTERS = (plan.set_infer_fuse, plan.set_infer_fuse_dwpw, plan.set_infer_fuse_msrb, plan.set_infer_fuse_bneck)


@pytest.fixture(autouse=True)
def _switches_back():
    yield
    for f in SETTERS:
        f(None)


def _fwd(m, x, setting):
    """setting: "off" | "bneck" | "full" (all four passes).  Returns (output, plan); the key ends (.., bneck, msrb, dwpw, fuse)."""
    flags = {"off": (False, False, False, False), "bneck": (False, False, False, True), "full": (True, True, True, True)}[setting]
    for f, on in zip(SETTERS, flags):
        f(on)
    with torch.no_grad():
        y = m(x).clone()
    p = [p for k, p in m.__dict__["_engine"].plans.items() if k[0] == tuple(x.shape) and tuple(k[-4:]) == (flags[3], flags[2], flags[1], flags[0])]
    assert len(p) == 1
    return y, p[0]


def _check_forms(tag, m, ref, x, dev, n_bneck):
    with torch.no_grad():
        y64 = ref(x.double())
        y64 = y64[-1] if isinstance(y64, (tuple, list)) else y64
    xg = x.to(dev)
    for form in ("eval", "deployed"):
        if form == "deployed":
            m.deploy_model()
        y_u, p_u = _fwd(m, xg, "off")
        assert p_u.pb.n_fused_bneck == 0
        for setting in ("bneck", "full"):
            y_f, p_f = _fwd(m, xg, setting)
            assert p_f.pb.n_fused_bneck == n_bneck == sum(r["op"] == BNECK for r in p_f.pb.recs)
            if form == "deployed":
                assert not any(r["op"] == FINALIZE for r in p_f.pb.recs)
            _compare(f"bneck_{tag}_{form}_{setting}", y_f, y_u, y64)
            assert torch.equal(_fwd(m, xg, setting)[0], y_f)             # second run: tables and weight scratch reused, same bits


@pytest.mark.parametrize("size", [256, 224])
def test_variant_a_eval_and_deployed(dev, size):
    m, ref = _pair("A", size, 21)
    m.to(dev).eval()
    _check_forms(f"A_{size}", m, ref, synth.synth_images(2, size, 5), dev, 13)


def test_reduction_2_eval_and_deployed(dev):
    cfg = litehandnet_cfg("A", image_size=64, reduction=2)
    cfg.MODEL["ca_dropout"] = 0.0
    ref = torch_ref.get_model(cfg, p_drop=0.0)
    sd = synth.synth_state_dict(ref, 23)
    ref.load_state_dict(sd)
    m = get_model(cfg)
    m.load_state_dict(sd)
    m.to(dev).eval()
    y, p = _fwd(m, synth.synth_images(2, 64, 5).to(dev), "bneck")
    assert {r["mids"][0].C for r in p.pb.recs if r["op"] == BNECK} == {64}
    _check_forms("A_r2_64", m, ref.double().eval(), synth.synth_images(2, 64, 5), dev, 13)


def test_variant_a_deployed_golden(dev, golden_dir):
    """The fused deployed forward against the reference's recorded heat maps, at the tolerance test_deploy_model_golden holds the
    unfused forward to.  The 64 x 64 image takes the kernel down to 4 x 4 and 2 x 2 maps."""
    g = np.load(os.path.join(golden_dir, "model_A_64_deploy.npz"))
    m = get_model(litehandnet_cfg("A"))
    m.load_state_dict(synth.synth_state_dict(m, int(g["weights_seed"])))
    m.to(dev).eval()
    x = synth.synth_images(2, 64, int(g["seed"])).to(dev)
    y_eval, p = _fwd(m, x, "bneck")
    assert p.pb.n_fused_bneck == 13 and {r["x"].H for r in p.pb.recs if r["op"] == BNECK} == {16, 8, 4, 2}
    m.deploy_model()
    y, q = _fwd(m, x, "bneck")
    assert q.pb.n_fused_bneck == 13
    ref = g["heatmap"]
    assert np.abs(y.cpu().numpy() - ref).max() <= FWD_TOL * np.abs(ref).max()
    assert _rel(y, y_eval) < 1e-4


def test_tables_follow_the_parameters(dev):
    """The table cache covers t1..t3 and the tap-major copy of the 3x3 weights: after the BatchNorm behind t2 or the 3x3 weights
    change, or a train-mode run moves the running statistics, the next fused eval forward equals one from a freshly built plan."""
    m, _ = _pair("A", 64, 41)
    m.to(dev).eval()
    x = synth.synth_images(2, 64, 7).to(dev)
    y1, p = _fwd(m, x, "bneck")
    y1b, _ = _fwd(m, x, "bneck")
    assert torch.equal(y1, y1b) and p._table_sig is not None

    def fresh():
        m.__dict__.pop("_engine", None)
        return _fwd(m, x, "bneck")[0]
    rec = next(r for r in p.pb.recs if r["op"] == BNECK)
    bn2 = next(r["bn"] for r in p.pb.recs if r["op"] == FINALIZE and r["out"].buf == rec["mids"][1].buf)     # the BatchNorm behind t2
    with torch.no_grad():
        bn2.bias.add_(0.5)
        bn2.running_var.mul_(2.0)
    y2, _ = _fwd(m, x, "bneck")
    assert not torch.equal(y2, y1)
    assert torch.equal(y2, fresh())
    _fwd(m, x, "bneck")                                # (tables current again)
    with torch.no_grad():
        rec2 = next(r for r in m.__dict__["_engine"].plans[next(iter(m.__dict__["_engine"].plans))].pb.recs if r["op"] == BNECK)
        rec2["convs"][1].weight.mul_(1.5)              # the scratch holds a copy of these
    y2w, _ = _fwd(m, x, "bneck")
    assert not torch.equal(y2w, y2)
    assert torch.equal(y2w, fresh())
    m.train()
    with torch.no_grad():                              # train-mode BatchNorm under no_grad: runs the unfused plan, moves the statistics
        m(synth.synth_images(4, 64, 8).to(dev))
    m.eval()
    y3, _ = _fwd(m, x, "bneck")
    assert not torch.equal(y3, y2w)
    assert torch.equal(y3, fresh())
    plan.invalidate_tables()
    assert torch.equal(_fwd(m, x, "bneck")[0], y3)


@pytest.mark.parametrize("variant", ["M", "B"])
def test_other_variants_eval(dev, variant):
    """Whatever the structural rule finds there (these trees have no 128 -> 32 / 64 -> 128 BottleNeck: nothing), the forward holds."""
    m, ref = _pair(variant, 64, 31)
    m.to(dev).eval()
    x = synth.synth_images(2, 64, 6)
    with torch.no_grad():
        y64 = ref(x.double())
        y64 = y64[-1] if isinstance(y64, (tuple, list)) else y64
    xg = x.to(dev)
    y_u, _ = _fwd(m, xg, "off")
    y_f, p_f = _fwd(m, xg, "bneck")
    assert p_f.pb.n_fused_bneck == sum(r["op"] == BNECK for r in p_f.pb.recs)
    _compare(f"bneck_{variant}_64_eval", y_f, y_u, y64)


def test_hipgraph_replay_matches_plain_launches(dev, tmp_path):
    """LHN_GRAPH=1 in a fresh child process: the fused eval forward replayed as a hipGraph equals the plain-launch one."""
    outs = {}
    for mode in ("0", "1"):
        path = str(tmp_path / f"y{mode}.pt")
        env = dict(os.environ, LHN_GRAPH=mode)
        for name in ("LHN_INFER_FUSE", "LHN_INFER_FUSE_DWPW", "LHN_INFER_FUSE_MSRB", "LHN_INFER_FUSE_BNECK"):
            env.pop(name, None)
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bneck_graph_child.py"), path], env=env, capture_output=True,
                             text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        outs[mode] = torch.load(path)
    assert torch.equal(outs["0"], outs["1"])
