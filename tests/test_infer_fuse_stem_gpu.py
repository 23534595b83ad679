"""GPU: whole models with the stem inference fusion on (plan.set_infer_fuse_stem): everything after the stem's first convolution runs
as one launch (lhn_stem_tail_fwd).  The arbiter is the float64 oracle; the yardstick is the UNFUSED forward of the same process on
the same inputs, with the criterion of tests/test_infer_fuse_gpu.py (_compare): at most 3x the unfused distance from float64, floor
1e-4 of the heat maps' peak, argmax equal except at near-ties."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from litehandnet_amd import get_model, plan
from litehandnet_amd.config import litehandnet_cfg
from litehandnet_amd.plan import FINALIZE, STEMTAIL
import ablation_ref
from oracle import synth
from test_infer_fuse_gpu import _compare, _pair
from test_model_gpu import FWD_TOL, _rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# in the order of the plan key's tail, from its end: (.., stem, bf16x3, bneck, msrb, dwpw, fuse)
SETTERS = (plan.set_infer_fuse, plan.set_infer_fuse_dwpw, plan.set_infer_fuse_msrb, plan.set_infer_fuse_bneck, plan.set_infer_bf16x3,
           plan.set_infer_fuse_stem)
FLAGS = {"off": (False,) * 6, "stem": (False,) * 5 + (True,), "everything": (True,) * 6}


@pytest.fixture(autouse=True)
def _switches_back():
    yield
    for f in SETTERS:
        f(None)


def _fwd(m, x, setting):
    """setting: "off" | "stem" | "everything" (all six switches).  Returns (output, plan)."""
    flags = FLAGS[setting]
    for f, on in zip(SETTERS, flags):
        f(on)
    with torch.no_grad():
        y = m(x).clone()
    p = [p for k, p in m.__dict__["_engine"].plans.items() if k[0] == tuple(x.shape) and tuple(k[-6:]) == tuple(reversed(flags))]
    assert len(p) == 1
    return y, p[0]


def _y64(ref, x):
    with torch.no_grad():
        y64 = ref(x.double())
    return y64[-1] if isinstance(y64, (tuple, list)) else y64


def _ks(p):
    return [r["K"] for r in p.pb.recs if r["op"] == STEMTAIL]


@pytest.mark.parametrize("size", [256, 224])
def test_variant_a_eval_and_deployed(dev, size):
    m, ref = _pair("A", size, 21)
    m.to(dev).eval()
    x = synth.synth_images(2, size, 5)
    y64, xg = _y64(ref, x), x.to(dev)
    for form, K in (("eval", 0), ("deployed", 7)):
        if form == "deployed":
            m.deploy_model()
        y_u, p_u = _fwd(m, xg, "off")
        assert p_u.pb.n_fused_stem == 0
        for setting in ("stem", "everything"):
            y_f, p_f = _fwd(m, xg, setting)
            assert p_f.pb.n_fused_stem == 1 and _ks(p_f) == [K]
            if form == "deployed" and setting == "stem":
                assert not any(r["op"] == FINALIZE for r in p_f.pb.recs)
            _compare(f"stem_A_{size}_{form}_{setting}", y_f, y_u, y64)
            assert torch.equal(_fwd(m, xg, setting)[0], y_f)             # second run: tables and weight scratch reused, same bits


def test_variant_a_deployed_golden(dev, golden_dir):
    """The fused deployed forward against the reference's recorded heat maps, at the tolerance test_deploy_model_golden holds the
    unfused forward to."""
    g = np.load(os.path.join(golden_dir, "model_A_64_deploy.npz"))
    m = get_model(litehandnet_cfg("A"))
    m.load_state_dict(synth.synth_state_dict(m, int(g["weights_seed"])))
    m.to(dev).eval()
    x = synth.synth_images(2, 64, int(g["seed"])).to(dev)
    y_eval, p = _fwd(m, x, "stem")
    assert _ks(p) == [0]
    m.deploy_model()
    y, q = _fwd(m, x, "stem")
    assert _ks(q) == [7]
    ref = g["heatmap"]
    assert np.abs(y.cpu().numpy() - ref).max() <= FWD_TOL * np.abs(ref).max()
    assert _rel(y, y_eval) < 1e-4


@pytest.mark.parametrize("size", [64, 256])
def test_mynet_eval(dev, size):
    m, ref = _pair("M", size, 31)
    m.to(dev).eval()
    x = synth.synth_images(2, size, 6)
    y64, xg = _y64(ref, x), x.to(dev)
    y_u, _ = _fwd(m, xg, "off")
    y_f, p_f = _fwd(m, xg, "stem")
    assert p_f.pb.n_fused_stem == 1 and _ks(p_f) == [3]
    _compare(f"stem_M_{size}_eval", y_f, y_u, y64)
    assert torch.equal(_fwd(m, xg, "stem")[0], y_f)


@pytest.mark.parametrize("variant", ["B", "X"])
def test_other_variants_eval(dev, variant):
    """Whatever the structural rule finds there (B: nothing -- its branch1 is 1x1 -> depthwise -> 1x1), the forward holds."""
    if variant == "X":      # hourglass_ablation: its float64 arbiter is tests/ablation_ref.py
        cfg = litehandnet_cfg("X", image_size=64)
        cfg.MODEL["ca_dropout"] = 0.0
        ref = ablation_ref.get_model(cfg, p_drop=0.0)
        sd = synth.synth_state_dict(ref, 31)
        ref.load_state_dict(sd)
        m, ref = get_model(cfg), ref.double().eval()
        m.load_state_dict(sd)
    else:
        m, ref = _pair(variant, 64, 31)
    m.to(dev).eval()
    x = synth.synth_images(2, 64, 6)
    y64, xg = _y64(ref, x), x.to(dev)
    y_u, _ = _fwd(m, xg, "off")
    y_f, p_f = _fwd(m, xg, "stem")
    assert p_f.pb.n_fused_stem == len(_ks(p_f)) and (variant != "B" or p_f.pb.n_fused_stem == 0)
    _compare(f"stem_{variant}_64_eval", y_f, y_u, y64)


def test_tables_follow_the_parameters(dev):
    """The table cache covers the tables of u and v and the tap-major copy of the 3x3 weights: after the BatchNorm behind u or the
    3x3 weights change, or a train-mode run moves the running statistics, the next fused eval forward equals one from a fresh plan."""
    m, _ = _pair("A", 64, 41)
    m.to(dev).eval()
    x = synth.synth_images(2, 64, 7).to(dev)
    y1, p = _fwd(m, x, "stem")
    y1b, _ = _fwd(m, x, "stem")
    assert torch.equal(y1, y1b) and p._table_sig is not None

    def fresh():
        m.__dict__.pop("_engine", None)
        return _fwd(m, x, "stem")[0]
    rec = next(r for r in p.pb.recs if r["op"] == STEMTAIL)
    bn_u = next(r["bn"] for r in p.pb.recs if r["op"] == FINALIZE and r["out"].buf == rec["u"].buf)     # the BatchNorm behind u
    with torch.no_grad():
        bn_u.bias.add_(0.5)
        bn_u.running_var.mul_(2.0)
    y2, _ = _fwd(m, x, "stem")
    assert not torch.equal(y2, y1)
    assert torch.equal(y2, fresh())
    _fwd(m, x, "stem")                                 # (tables current again)
    with torch.no_grad():
        rec2 = next(r for r in m.__dict__["_engine"].plans[next(iter(m.__dict__["_engine"].plans))].pb.recs if r["op"] == STEMTAIL)
        rec2["convs"][1].weight.mul_(1.5)              # the scratch holds a copy of these
    y2w, _ = _fwd(m, x, "stem")
    assert not torch.equal(y2w, y2)
    assert torch.equal(y2w, fresh())
    m.train()
    with torch.no_grad():                              # train-mode BatchNorm under no_grad: runs the unfused plan, moves the statistics
        m(synth.synth_images(4, 64, 8).to(dev))
    m.eval()
    y3, _ = _fwd(m, x, "stem")
    assert not torch.equal(y3, y2w)
    assert torch.equal(y3, fresh())
    plan.invalidate_tables()
    assert torch.equal(_fwd(m, x, "stem")[0], y3)


def test_hipgraph_replay_matches_plain_launches(dev, tmp_path):
    """LHN_GRAPH=1 in a fresh child process: the fused eval forward replayed as a hipGraph equals the plain-launch one."""
    outs = {}
    for mode in ("0", "1"):
        path = str(tmp_path / f"y{mode}.pt")
        env = dict(os.environ, LHN_GRAPH=mode)
        for name in ("LHN_INFER_FUSE", "LHN_INFER_FUSE_DWPW", "LHN_INFER_FUSE_MSRB", "LHN_INFER_FUSE_BNECK", "LHN_INFER_BF16X3", "LHN_INFER_FUSE_STEM"):
            env.pop(name, None)
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stem_graph_child.py"), path], env=env, capture_output=True,
                             text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        outs[mode] = torch.load(path)
    assert torch.equal(outs["0"], outs["1"])
