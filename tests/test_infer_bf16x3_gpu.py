"""GPU: whole models with the split-bf16 switch on (plan.set_infer_bf16x3): the eligible dense 3x3 convolutions of an inference plan
run on the bf16 MFMA with a three-term split (lhn_conv_kxk_fwd_bf16x3), alone and on top of the four fusion passes.  The arbiter is
the float64 oracle; the bar is the project's forward rule, max(1e-4, 3 x the error of the reference's own float32 run on the CPU) of the
heat maps' peak; against the switch-off forward of the same process the argmax coordinates are equal except at near-ties of the float64
map (the criterion of tests/test_infer_fuse_gpu.py).
With the 32 -> 32 class on the bf16 MFMA as well, variant A at 256 x 256 measured 1.46e-4 (eval) / 1.55e-4 (deployed) against the 1e-4
bar while the kernel suite was green; the class was taken out of plan.bf16x3_eligible (plan.BF16X3_LEFT_OUT) and the bar stayed."""
import copy

import numpy as np
import pytest
import torch

from conftest import parity_record
from litehandnet_amd import heatmap, plan
from litehandnet_amd.plan import BNECK, KXK
from oracle import synth
from test_infer_fuse_gpu import _pair
from test_model_gpu import _rel

pytestmark = pytest.mark.gpu
SETTERS = (plan.set_infer_fuse, plan.set_infer_fuse_dwpw, plan.set_infer_fuse_msrb, plan.set_infer_fuse_bneck, plan.set_infer_bf16x3)
SETTINGS = {"off": (False,) * 5, "bf16x3": (False, False, False, False, True), "full": (True, True, True, True, False),
            "full+bf16x3": (True,) * 5}


@pytest.fixture(autouse=True)
def _switches_back():
    yield
    for f in SETTERS:
        f(None)


def _fwd(m, x, setting):
    """Returns (output, plan); the plan key is (shape, backward, p_drop, device, bf16x3, bneck, msrb, dwpw, fuse)."""
    flags = SETTINGS[setting]
    for f, on in zip(SETTERS, flags):
        f(on)
    with torch.no_grad():
        y = m(x).clone()
    p = [p for k, p in m.__dict__["_engine"].plans.items() if k[0] == tuple(x.shape) and tuple(k[-5:]) == flags[::-1]]
    assert len(p) == 1
    return y, p[0]


def _last(y):
    y = y[-1] if isinstance(y, (tuple, list)) else y
    return y[:, -1] if y.dim() == 5 else y                 # stacked hourglass [N, S, K, H, W]: the last stack is the prediction


def _oracle(ref, x):
    """(float64 heat maps, error of the reference's float32 run on the CPU)."""
    with torch.no_grad():
        y64 = _last(ref(x.double()))
        y32 = _last(copy.deepcopy(ref).float()(x))
    return y64, _rel(y32, y64)


def _compare(tag, y_on, y_off, y64, e32):
    y_on, y_off = _last(y_on), _last(y_off)
    e_on, e_off = _rel(y_on, y64), _rel(y_off, y64)
    bar = max(1e-4, 3 * e32)
    scale = float(y64.abs().max())
    n, k, h, w = y64.shape
    pn, _ = heatmap._get_max_preds(y_on.contiguous())
    pf, _ = heatmap._get_max_preds(y_off.contiguous())
    pn, pf = pn.cpu().numpy(), pf.cpu().numpy()
    diff = ~(pn == pf).all(-1)
    flat = y64.numpy().reshape(n, k, -1)
    idx = (pn[..., 1] * w + pn[..., 0]).astype(np.int64).clip(0)
    gap = flat.max(-1) - np.take_along_axis(flat, idx[..., None], -1)[..., 0]
    print(f"infer_bf16x3 {tag}: on {e_on:.3e} off {e_off:.3e} float32 on the CPU {e32:.3e} bar {bar:.3e}; argmax differs at {int(diff.sum())} of {n * k}")
    parity_record(f"infer_bf16x3/{tag}", heatmap_err_on=e_on, heatmap_err_off=e_off, heatmap_err_ref_fp32=e32, heatmap_bar=bar,
                  argmax_disagree_vs_off=int(diff.sum()), keypoints=int(n * k))
    assert e_on <= bar, (tag, e_on, e_off, bar)
    assert (gap[diff] <= 2 * max(e_on, 1e-6) * scale).all(), (tag, float(gap[diff].max()), e_on * scale)


def _check(tag, m, xg, y64, e32, n_alone):
    y_off, p_off = _fwd(m, xg, "off")
    assert p_off.pb.n_bf16x3 == 0
    y_full, _ = _fwd(m, xg, "full")
    for setting, base in (("bf16x3", y_off), ("full+bf16x3", y_full)):
        y_on, p_on = _fwd(m, xg, setting)
        marked = [r for r in p_on.pb.recs if r["op"] == KXK and r.get("bf16x3")]
        want = n_alone - (1 if any(r["op"] == BNECK and r["mids"][0].C == 64 for r in p_on.pb.recs) else 0)      # A's 64 -> 64 sits in a BNECK
        assert p_on.pb.n_bf16x3 == len(marked) == want, (tag, setting, len(marked), want)
        _compare(f"{tag}_{setting}", y_on, base, y64, e32)
        assert torch.equal(_fwd(m, xg, setting)[0], y_on)          # second run: tables and split weights reused, same bits


@pytest.mark.parametrize("size", [256, 64])
def test_variant_a_eval_and_deployed(dev, size):
    m, ref = _pair("A", size, 21)
    m.to(dev).eval()
    x = synth.synth_images(2, size, 5)
    y64, e32 = _oracle(ref, x)
    _check(f"A_{size}_eval", m, x.to(dev), y64, e32, 10)
    m.deploy_model()
    _check(f"A_{size}_deployed", m, x.to(dev), y64, e32, 10)


@pytest.mark.parametrize("variant, n_alone", [("M", 9), ("H", 31)])
def test_other_variants_eval(dev, variant, n_alone):
    m, ref = _pair(variant, 128, 31)
    m.to(dev).eval()
    x = synth.synth_images(2, 128, 6)
    y64, e32 = _oracle(ref, x)
    _check(f"{variant}_128_eval", m, x.to(dev), y64, e32, n_alone)


def test_train_mode_and_backward_plans_stay_fp32(dev):
    """Train-mode BatchNorm under no_grad needs batch statistics, and a plan with a backward needs the fp32 kernels' gradients: neither
    carries the flag, whatever the switch says."""
    m, _ = _pair("A", 64, 41)
    m.to(dev).train()
    plan.set_infer_bf16x3(True)
    x = synth.synth_images(2, 64, 7).to(dev)
    with torch.no_grad():
        m(x)
    m(x).sum().backward()
    plans = list(m.__dict__["_engine"].plans.values())
    assert len(plans) == 2 and all(p.pb.n_bf16x3 == 0 and not any(r.get("bf16x3") for r in p.pb.recs) for p in plans)


def test_split_weights_follow_the_parameters(dev):
    """The scratch is rebuilt with the tables: after the 3x3 weights change, the next forward equals one from a freshly built plan."""
    m, _ = _pair("A", 64, 41)
    m.to(dev).eval()
    x = synth.synth_images(2, 64, 7).to(dev)
    y1, p = _fwd(m, x, "bf16x3")
    assert torch.equal(_fwd(m, x, "bf16x3")[0], y1)
    rec = next(r for r in p.pb.recs if r["op"] == KXK and r.get("bf16x3"))
    with torch.no_grad():
        rec["conv"].weight.mul_(1.5)
    y2, _ = _fwd(m, x, "bf16x3")
    assert not torch.equal(y2, y1)
    m.__dict__.pop("_engine", None)
    assert torch.equal(_fwd(m, x, "bf16x3")[0], y2)
