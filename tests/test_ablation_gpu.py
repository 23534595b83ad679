"""GPU: the `hourglass_ablation` family (litehandnet_amd/hourglass_ablation.py) against its float64 restatement
(tests/ablation_ref.py, proved bit-equal to the real reference by tests/golden/make_golden_ablation.py).  Blocks: ME_att for
every ca_type and a Residual with rca, with the block bars of tests/test_model_gpu.py.  Networks: the six model_X<tag>_128
fixtures (heatmap, loss, gradient norms, a running mean, argmax), the cbam and nomsrb networks at 224x224, eval mode after two
training steps, and dropout live with shared masks."""
import os

import numpy as np
import pytest
import torch

import ablation_ref
from conftest import parity_record
from litehandnet_amd.config import litehandnet_cfg
from oracle import heatmap_np as onp
from oracle import synth, torch_ref
from test_dropout_gpu import _block as _dropout_block
from test_model_gpu import FWD_TOL, MODEL_GRAD_FACTOR, MODEL_GRAD_FLOOR, _check_block, _x

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("hw", [16, 14])
@pytest.mark.parametrize("ca_type", ["ca", "se", "1x1", "identity", "cbam"])
def test_me_att_block(dev, ca_type, hw):
    from litehandnet_amd import hourglass_ablation as ha
    _check_block(ha.ME_att(128, 128, ca_type, p_drop=0.0), ablation_ref.ME_att(128, 128, ca_type, p_drop=0.0), _x(2, 128, hw, hw, seed=hw),
                 dev, seed=60 + hw)


@pytest.mark.parametrize("hw", [16, 14])
def test_residual_rca_block(dev, hw):
    from litehandnet_amd import hourglass_ablation as ha
    _check_block(ha.Residual(128, 128, 1, 2, rca=True, p_drop=0.0), ablation_ref.Residual(128, 128, 1, 2, True, 0.0),
                 _x(2, 128, hw, hw, seed=hw + 1), dev, seed=70 + hw)


def _model_case(dev, golden_dir, tag):
    """test_model_gpu._model_case's procedure with tests/ablation_ref.py as the float64 arbiter: the HIP fp32 run must be as close
    to float64 as the REFERENCE's own fp32 run (the fixture) is, up to a factor 3 (floors 1e-4 heatmap, 1e-3 gradient norms);
    argmax coordinates equal the float64 ones wherever the reference's fp32 run agrees with float64."""
    from litehandnet_amd import get_loss, get_model, heatmap
    g = np.load(os.path.join(golden_dir, f"model_X{tag}_128.npz"))
    cfg = litehandnet_cfg("X", image_size=int(g["size"]), **ablation_ref.TAGS[tag])
    cfg.MODEL["ca_dropout"] = 0.0
    n, size, seed = int(g["n"]), int(g["size"]), int(g["seed"])
    hs = size // 4
    j = synth.synth_joints(n, 21, size, seed + 1)
    tgt = np.stack([onp.msra_generate_target(a, np.ones_like(a), [size, size], [hs, hs])[0] for a in j])
    tw = torch.from_numpy(g["target_weight"])
    ref = ablation_ref.get_model(cfg, p_drop=0.0)
    sd = synth.synth_state_dict(ref, seed)
    ref.load_state_dict(sd)
    ref = ref.double().train()
    y64 = ref(synth.synth_images(n, size, seed).double())
    l64 = cfg.LOSS.loss_weight[0] * torch_ref.distance_loss(y64, torch.from_numpy(tgt).double(), tw.double())
    l64.backward()
    l64 = l64.detach()
    y64n = y64.detach().numpy()
    scale = np.abs(y64n).max()
    ref32_err = np.abs(g["heatmap"] - y64n).max() / scale
    m = get_model(cfg)
    m.load_state_dict(sd)
    m.to(dev).train()
    y = m(synth.synth_images(n, size, seed).to(dev))
    err = np.abs(y.detach().cpu().numpy() - y64n).max() / scale
    loss, _ = get_loss(cfg)(y, {"target": torch.from_numpy(tgt), "target_weight": tw})
    loss.backward()
    gn32 = dict(zip(g["grad_keys"].tolist(), g["grad_norms"].tolist()))
    gn64 = {k: float(p.grad.norm()) for k, p in ref.named_parameters()}
    floor = 1e-3 * max(gn64.values())
    errs = {k: abs(float(p.grad.norm()) - gn64[k]) / (gn64[k] + floor) for k, p in m.named_parameters()}
    errs32 = {k: abs(gn32[k] - gn64[k]) / (gn64[k] + floor) for k in gn64}
    worst, worst32 = max(errs.values()), max(errs32.values())
    top = sorted(errs, key=lambda k: -errs[k])[:3]
    bk = str(g["bn_key"])
    rm64 = ref.state_dict()[bk].numpy()
    rm_err, rm_tol = np.abs(m.state_dict()[bk].cpu().numpy() - rm64).max(), max(1e-5, 3 * np.abs(g["bn_running_mean"] - rm64).max())
    p, _ = heatmap._get_max_preds(y.detach().contiguous())
    p64, _ = onp.get_max_preds(np.ascontiguousarray(y64n).astype(np.float32))
    p32, _ = onp.get_max_preds(np.ascontiguousarray(g["heatmap"]))
    same32 = (p32 == p64).all(-1)
    pn = p.cpu().numpy()
    loss_err, loss_err32 = abs(float(loss.detach()) - float(l64)), abs(float(g["loss"]) - float(l64))
    parity_record(f"model_X{tag}_128_golden", heatmap_err=err, heatmap_err_ref_fp32=ref32_err, heatmap_bar=max(3 * ref32_err, 1e-4),
                  loss_err=loss_err / abs(float(l64)), loss_err_ref_fp32=loss_err32 / abs(float(l64)),
                  grad_norm_worst=worst, grad_norm_ref_fp32_worst=worst32, grad_norm_bar=max(MODEL_GRAD_FACTOR * worst32, MODEL_GRAD_FLOOR),
                  grad_norm_worst_params=[f"{k}: hip {errs[k]:.3e} / reference-fp32 {errs32[k]:.3e}" for k in top],
                  running_mean_err=rm_err, running_mean_bar=rm_tol,
                  argmax_disagree_vs_f64=int((~(pn == p64).all(-1)).sum()), argmax_ref_fp32_disagree_vs_f64=int((~same32).sum()))
    print(f"[X{tag}] heatmap err vs f64: hip {err:.2e} / reference-fp32 {ref32_err:.2e}; grad-norm err: hip {worst:.2e} / "
          f"reference-fp32 {worst32:.2e} ({top[0]}); loss err hip {loss_err:.2e} / reference-fp32 {loss_err32:.2e}")
    assert err <= max(3 * ref32_err, 1e-4), (err, ref32_err)
    assert loss_err <= max(3 * loss_err32, 1e-5 * abs(float(l64)))
    assert worst <= max(MODEL_GRAD_FACTOR * worst32, MODEL_GRAD_FLOOR), (worst, worst32, top)
    assert rm_err <= rm_tol
    assert (pn == p64).all(-1)[same32].all()


@pytest.mark.parametrize("tag", list(ablation_ref.TAGS))
def test_model_X_128_golden(dev, golden_dir, tag):
    _model_case(dev, golden_dir, tag)


@pytest.mark.parametrize("tag", ["cbam", "nomsrb"])
def test_model_X_224_input(dev, tag):
    """config/hourglass_ablation/freihand/*.py train at 224x224: maps 56 / 28 / 14 / 7.  Forward and gradients vs float64, as
    test_model_gpu.test_model_224_input."""
    from litehandnet_amd import get_model
    cfg = litehandnet_cfg("X", image_size=224, **ablation_ref.TAGS[tag])
    cfg.MODEL["ca_dropout"] = 0.0
    _check_block(get_model(cfg), ablation_ref.get_model(cfg, p_drop=0.0), synth.synth_images(1, 224, 22), dev, seed=31, no_dx=True,
                 grad_tol=2e-2)


def test_model_X_cbam_eval_after_training(dev):
    """Two training steps move the running statistics; eval mode (its own plan, running-statistics tables) then agrees with the
    restatement in eval mode carrying the HIP model's state."""
    from litehandnet_amd import get_model
    cfg = litehandnet_cfg("X", image_size=128, ca_type="cbam")
    cfg.MODEL["ca_dropout"] = 0.0
    m, ref = get_model(cfg), ablation_ref.get_model(cfg, p_drop=0.0)
    sd = synth.synth_state_dict(ref, 57)
    m.load_state_dict(sd)
    ref.load_state_dict(sd)
    m.to(dev).train()
    ref.train()
    for step in range(2):
        x = synth.synth_images(2, 128, 58 + step)
        m(x.to(dev)).sum().backward()
        ref(x)
    for k, v in m.state_dict().items():
        if k.endswith("running_mean") or k.endswith("running_var"):
            assert torch.allclose(v.cpu(), ref.state_dict()[k], rtol=1e-3, atol=1e-4), k
        if k.endswith("num_batches_tracked"):
            assert int(v) == 2, k
    ref.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    m.eval()
    ref = ref.double().eval()
    x = synth.synth_images(2, 128, 61)
    with torch.no_grad():
        y, y64 = m(x.to(dev)).cpu().double(), ref(x.double())
        y32 = ref.float()(x).double()
    err, e32 = float((y - y64).abs().max() / y64.abs().max()), float((y32 - y64).abs().max() / y64.abs().max())
    parity_record("model_Xcbam_eval", heatmap_err=err, heatmap_err_ref_fp32=e32, heatmap_bar=max(FWD_TOL, 3 * e32))
    assert err <= max(FWD_TOL, 3 * e32), (err, e32)


def test_model_X_rca_with_dropout(dev):
    """nn.Dropout(p=0.3) of all eight attentions live, the masks shared with the restatement through Engine.mask_fn."""
    from litehandnet_amd import get_model
    cfg = litehandnet_cfg("X", image_size=128, rca=True)
    ours, ref = get_model(cfg), ablation_ref.get_model(cfg, p_drop=0.3)
    masks = _dropout_block(ours, ref, synth.synth_images(8, 128, 9), dev, seed=84, no_dx=True, grad_tol=3e-2)
    assert len(masks) == 8 and all(0 < float((v == 0).float().mean()) < 1 for v in masks.values())
