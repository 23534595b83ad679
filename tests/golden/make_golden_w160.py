"""Fixture of `mynet` at input_channel = 160 (the reference's config/mynet/w160 files).  RUNS ONLY IN THE BUILD CONTAINER (needs the
reference, see make_golden.py).

  model_M160_64.npz      the REAL reference's fp32 forward + TopdownHeatmapLoss + backward at batch 4 on 64 x 64 with weights
                         synth_state_dict(seed): heat map, loss, gradient norms, the first BatchNorm's running statistics
                         (make_golden._model_case; the oracle must agree or nothing is written).  3,490,101 parameters.
  model_M160_64_f64.npz  the same case in float64 (make_golden_f64.heatmap_summary, loss, gradient norms), which
                         tests/test_oracle_golden._run_case holds the float64 oracle to.

    python tests/golden/make_golden_w160.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden import _load_reference, _model_case, _no_dropout  # noqa: E402
from make_golden_f64 import heatmap_summary  # noqa: E402
from litehandnet_amd.config import litehandnet_cfg  # noqa: E402
from oracle import heatmap_np as onp  # noqa: E402
from oracle import synth, torch_ref  # noqa: E402

TAG, N, SIZE, SEED = "M160_64", 4, 64, 61


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    ref_models, _, RefLoss, _, _, _ = _load_reference()
    cfgA = litehandnet_cfg("A")
    out = {"ref_loss": RefLoss(cfgA), "ora_loss": torch_ref.TopdownHeatmapLoss(cfgA)}
    cfg = litehandnet_cfg("M", channels=160)
    rM, oM = ref_models.get_model(cfg), torch_ref.get_model(cfg)
    assert list(rM.state_dict()) == list(oM.state_dict())
    assert sum(p.numel() for p in rM.parameters()) == 3490101
    _model_case(rM, oM, N, SIZE, SEED, TAG, out)

    g = np.load(os.path.join(HERE, f"model_{TAG}.npz"))
    r = ref_models.get_model(cfg)
    r.load_state_dict(synth.synth_state_dict(r, SEED))
    r = r.double().train()
    _no_dropout(r)
    y = r(synth.synth_images(N, SIZE, SEED).double())
    f64 = heatmap_summary(y.detach().numpy(), g["heatmap"])
    hs = SIZE // 4
    j = synth.synth_joints(N, 21, SIZE, SEED + 1)
    tgt = np.stack([onp.msra_generate_target(a, np.ones_like(a), [SIZE, SIZE], [hs, hs])[0] for a in j])
    meta = {"target": torch.from_numpy(tgt).double(), "target_weight": torch.from_numpy(g["target_weight"]).double()}
    loss, _ = out["ref_loss"](y, meta)
    loss.backward()
    keys = sorted(k for k, _ in r.named_parameters())
    assert keys == g["grad_keys"].tolist()
    gn = dict((k, float(p.grad.norm())) for k, p in r.named_parameters())
    f64.update(loss=np.float64(float(loss.detach())), grad_keys=np.array(keys), grad_norms=np.array([gn[k] for k in keys], np.float64))
    np.savez_compressed(os.path.join(HERE, f"model_{TAG}_f64.npz"), **f64)
    print(f"written model_{TAG}.npz, model_{TAG}_f64.npz; fp32 fixture vs float64 reference "
          f"{float(f64['heatmap_f32_err']) / float(f64['heatmap_absmax']):.2e} of the peak")


if __name__ == "__main__":
    main()
