"""GPU: `mynet` at input_channel = 160, the third width of the reference's configs (config/mynet/w160/_2_*, _6_*, _8_*, _9_*, _11_*).
Its dense 3x3 are 160 -> 160 (BasicBlock, stride 1 and 2) and 40 -> 40 (BottleNeck's inner convolution and the stem's branch, 40 =
160 / 4), its stem opens with 3 -> 40; tests/test_kxk160_gpu.py and tests/test_stem40_gpu.py hold those kernels to float64 per
element.  Here the blocks at this width and the whole network on a 64 x 64 image, batch 4, as tests/test_width256_models_gpu.py does
at 256: training forward, gradients and BatchNorm statistics against the float64 oracle (bars: 3x the reference's own fp32 error per
tensor), the real reference's fixture, eval forward, and one Trainer step.
`hourglass_ablation` shares these blocks and is checked the same way; variant A is not served at this width and must say so.
On a library without the width-160 instances every test here but the last stops with "unsupported channels" or "Cout=40".

Seeds (weights / images) of the whole-network check, measured on the CPU from the oracle's fp32 run against its float64 run before any
GPU run (forward error of the peak; worst and median parameter-gradient error as _check_block measures them): 61 / 60: 1.0e-4, 2.6e-2,
8.0e-3 -- used; 63 / 62: 8.8e-5, 4.3e-2, 1.6e-2; 65 / 64: 1.5e-4, 6.0e-2, 9.1e-3; 67 / 66: 1.3e-4, 1.7e-2, 7.4e-3 -- measured alongside
and not used.  At every seed the forward error is at FWD_TOL or above, so the 3x rule binds there; the network is as badly conditioned
at batch 4 on 64 x 64 as the 256-wide ones (test_width256_models_gpu.py)."""
import numpy as np
import pytest
import torch

import ablation_ref
from litehandnet_amd import _lib, plan
from litehandnet_amd.config import litehandnet_cfg
from oracle import heatmap_np as onp
from oracle import synth, torch_ref
from test_model_gpu import FWD_TOL, _check_block, _model_case, _rel, _x

pytestmark = pytest.mark.gpu
WIDTH = 160


def _cfg(**kw):
    cfg = litehandnet_cfg("M", channels=WIDTH, image_size=64, **kw)
    cfg.MODEL["ca_dropout"] = 0.0
    return cfg


def test_width_160_blocks(dev):
    """The blocks of pose_hg_ms_att.py at this width one by one (test_model_gpu.test_mynet_blocks at 128)."""
    from litehandnet_amd import pose_hg_ms_att as pm
    _check_block(pm.BottleNeck(WIDTH), torch_ref.MyBottleNeck(WIDTH), _x(4, WIDTH, 8, 8), dev, seed=1)
    for stride in (1, 2):
        _check_block(pm.BasicBlock(WIDTH, WIDTH, stride), torch_ref.MyBasicBlock(WIDTH, WIDTH, stride), _x(4, WIDTH, 8, 8), dev, seed=2)
    _check_block(pm.ME_att(WIDTH, WIDTH, p_drop=0.0), torch_ref.ME_att(WIDTH, WIDTH, 0.0), _x(4, WIDTH, 16, 16), dev, seed=4)
    _check_block(pm.my_pelee_stem(WIDTH), torch_ref._StemM(WIDTH), _x(2, 3, 64, 64), dev, seed=5, no_dx=True)


def test_width_160_training(dev):
    """Forward, parameter gradients and running statistics of the whole network against the float64 oracle; gradient bar 2e-2 as at
    256 (whole-network gradients, ReLU flips)."""
    from litehandnet_amd import get_model
    cfg = _cfg()
    _check_block(get_model(cfg), torch_ref.get_model(cfg, p_drop=0.0), synth.synth_images(4, 64, 60), dev, seed=61, no_dx=True, grad_tol=2e-2)


def test_width_160_training_ablation(dev):
    """hourglass_ablation is built from the same blocks (160 -> 160, 40 -> 40 and the 3 -> 40 stem) and runs at this width too: the check of
    test_width256_models_gpu.test_width_256_training_ablation, with its weights (40) and images (41) and its float64 arbiter."""
    from litehandnet_amd import get_model
    cfg = litehandnet_cfg("X", channels=WIDTH, image_size=64, ca_type="ca")
    cfg.MODEL["ca_dropout"] = 0.0
    _check_block(get_model(cfg), ablation_ref.get_model(cfg, p_drop=0.0), synth.synth_images(4, 64, 41), dev, seed=40, no_dx=True,
                 grad_tol=2e-2)


def test_width_160_variant_A_fails_loudly(dev):
    """Variant A at 160 contains an 80 -> 80 dense 3x3, which has no kernel: the first forward stops with the shape in the
    error, nothing falls back to anything."""
    from litehandnet_amd import get_model
    cfg = litehandnet_cfg("A", channels=WIDTH, image_size=64)
    m = get_model(cfg).to(dev).train()
    with pytest.raises(_lib.LhnError, match="unsupported channels Cin=80 Cout=80"):
        m(synth.synth_images(2, 64, 3).to(dev))


def test_width_160_reference_fixture(dev, golden_dir):
    """Forward + TopdownHeatmapLoss + backward against what the real reference computed (tests/golden/make_golden_w160.py)."""
    _model_case(dev, golden_dir, "M160_64", variant="M", channels=WIDTH)


def test_width_160_eval(dev):
    from litehandnet_amd import get_model
    cfg = _cfg()
    ref = torch_ref.get_model(cfg, p_drop=0.0)
    sd = synth.synth_state_dict(ref, 33)
    ref.load_state_dict(sd)
    ref = ref.double().eval()
    m = get_model(cfg)
    m.load_state_dict(sd)
    m.to(dev).eval()
    x = synth.synth_images(4, 64, 7)
    with torch.no_grad():
        y64 = ref(x.double())
        y = m(x.to(dev))
    assert _rel(y, y64) < FWD_TOL, ("eval", _rel(y, y64))
    recs = [r for pl in m.__dict__["_engine"].plans.values() for r in pl.pb.recs]
    assert any(r["op"] == plan.KXK and r["x"].C == WIDTH and r["out"].C == WIDTH for r in recs)
    assert not any(r["op"] in (plan.BNECK, plan.STEMTAIL) or r.get("bf16x3") for r in recs)


def test_width_160_trainer_step(dev):
    """One Trainer.step on synthetic targets: the training plan holds the 160 -> 160 and 40 -> 40 3x3 records (two per BasicBlock; one
    per BottleNeck and one in the stem), the loss equals the float64 oracle's at the forward bar, and the step moves the weights."""
    from litehandnet_amd import get_loss, get_model
    from litehandnet_amd import pose_hg_ms_att as pm
    from litehandnet_amd.train import Trainer
    cfg = _cfg()
    ref = torch_ref.get_model(cfg, p_drop=0.0)
    sd = synth.synth_state_dict(ref, 35)
    ref.load_state_dict(sd)
    ref = ref.double().train()
    m = get_model(cfg)
    m.load_state_dict(sd)
    m.to(dev).train()
    n, size = 4, 64
    x = synth.synth_images(n, size, 36)
    j = synth.synth_joints(n, 21, size, 37)
    t = np.stack([onp.msra_generate_target(a, np.ones_like(a), [size, size], [size // 4, size // 4])[0] for a in j])
    meta = {"target": torch.from_numpy(t), "target_weight": torch.ones(n, 21, 1)}
    trainer = Trainer(m, get_loss(cfg), lr=5e-4, world_size=1)
    before = trainer.fp.flat.clone()
    loss = float(trainer.step(x.to(dev), {k: v.to(dev) for k, v in meta.items()}).detach())
    l64, _ = torch_ref.TopdownHeatmapLoss(cfg)(ref(x.double()), {k: v.double() for k, v in meta.items()})
    assert np.isfinite(loss) and abs(loss - float(l64)) <= FWD_TOL * abs(float(l64)), (loss, float(l64))
    plans = list(m.__dict__["_engine"].plans.values())
    assert plans and all(pl.pb.with_backward for pl in plans)
    recs = [r for pl in plans for r in pl.pb.recs]
    nbb = sum(isinstance(b, pm.BasicBlock) for b in m.modules())
    nbn = sum(isinstance(b, pm.BottleNeck) for b in m.modules())
    kxk = [(r["x"].C, r["out"].C) for r in recs if r["op"] == plan.KXK]
    assert kxk.count((WIDTH, WIDTH)) == 2 * nbb > 0 and kxk.count((40, 40)) == nbn + 1 and len(kxk) == 2 * nbb + nbn + 1, kxk
    moved = (trainer.fp.flat - before).abs()
    assert torch.isfinite(trainer.fp.flat).all() and float(moved.max()) > 0
