"""Fixtures of the `hourglass_ablation` family.  RUNS ONLY WHERE THE REFERENCE CHECKOUT IS (make_golden.REF), as the other generators.

For each of the six networks (tests/ablation_ref.py: TAGS) the REAL reference (models.get_model) and the restatement
(tests/ablation_ref.py) get the same synthesised weights and run forward + TopdownHeatmapLoss + backward on seeded inputs,
N = 2 at 128x128 (maps 32 / 16 / 8 / 4), train-mode BatchNorm, dropout off.  Key lists, parameter counts, the forward, the
loss, every gradient and every buffer must be equal BIT FOR BIT; then the reference's results are stored as
model_X<tag>_128.npz in the format of make_golden._model_case.  init_weights_ablation.json holds the sha256 of the
reference's fresh state_dict() under a torch seed, per tag, as init_weights.json does for the other models.

    python tests/golden/make_golden_ablation.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import _load_reference, _no_dropout  # noqa: E402  (puts the repository root on sys.path)
from make_golden_r3 import SEED, state_digest  # noqa: E402
import ablation_ref  # noqa: E402
from litehandnet_amd import get_model as mirror_get_model  # noqa: E402
from litehandnet_amd.config import litehandnet_cfg  # noqa: E402
from oracle import heatmap_np as onp  # noqa: E402
from oracle import synth, torch_ref  # noqa: E402

N, SIZE = 2, 128
SEEDS = {"nomsrb": 51, "se": 52, "1x1": 53, "id": 54, "cbam": 55, "rca": 56}


def _run(model, lossmod, x, meta):
    model.train()
    _no_dropout(model)
    model.zero_grad()
    y = model(x)
    loss, _ = lossmod(y, meta)
    loss.backward()
    return dict(y=y.detach().numpy(), loss=float(loss), grads={k: p.grad.numpy().copy() for k, p in model.named_parameters()},
                bufs={k: v.numpy().copy() for k, v in model.state_dict().items()})


def model_fixture(tag, ref_models, RefLoss):
    cfg = litehandnet_cfg("X", image_size=SIZE, **ablation_ref.TAGS[tag])
    r, o = ref_models.get_model(cfg), ablation_ref.get_model(cfg)
    assert type(r).__name__ == "hourglass_ablation" and list(r.state_dict()) == list(o.state_dict())
    assert sum(p.numel() for p in r.parameters()) == ablation_ref.PARAMS[tag], tag
    seed = SEEDS[tag]
    sd = synth.synth_state_dict(r, seed)
    r.load_state_dict(sd)
    o.load_state_dict(sd)
    x = synth.synth_images(N, SIZE, seed)
    hs = SIZE // 4
    joints = synth.synth_joints(N, 21, SIZE, seed + 1)
    tgt = np.stack([onp.msra_generate_target(j, np.ones_like(j), [SIZE, SIZE], [hs, hs])[0] for j in joints])
    w = np.ones((N, 21, 1), np.float32)
    w[0, 3] = 0
    meta = {"target": torch.from_numpy(tgt), "target_weight": torch.from_numpy(w)}
    a, b = _run(r, RefLoss(cfg), x, meta), _run(o, torch_ref.TopdownHeatmapLoss(cfg), x, meta)
    assert np.array_equal(a["y"], b["y"]) and a["loss"] == b["loss"], tag
    for part in ("grads", "bufs"):
        assert list(a[part]) == list(b[part])
        for k in a[part]:
            assert np.array_equal(a[part][k], b[part][k]), (tag, part, k)
    keys = sorted(a["grads"])
    first_bn = sorted(k for k in a["bufs"] if k.endswith("running_mean"))[0]
    np.savez_compressed(
        os.path.join(HERE, f"model_X{tag}_{SIZE}.npz"),
        n=N, size=SIZE, seed=seed, heatmap=a["y"].astype(np.float32), loss=np.float64(a["loss"]),
        grad_keys=np.array(keys), grad_norms=np.array([float(np.linalg.norm(a["grads"][k].astype(np.float64))) for k in keys], np.float64),
        bn_key=np.array(first_bn), bn_running_mean=a["bufs"][first_bn],
        bn_running_var=a["bufs"][first_bn.replace("running_mean", "running_var")], target_weight=w,
        state_keys=np.array(list(sd)), state_shapes=np.array([",".join(map(str, v.shape)) for v in sd.values()]))
    print(f"[X{tag}] {ablation_ref.PARAMS[tag]} parameters, {len(sd)} tensors, loss {a['loss']:.6f}: restatement == reference bit for bit")


def init_fixture(ref_models):
    out = {"seed": SEED, "models": {}}
    for tag, kw in ablation_ref.TAGS.items():
        cfg = litehandnet_cfg("X", **kw)
        torch.manual_seed(SEED)
        r = ref_models.get_model(cfg)
        dig, sums = state_digest(r.state_dict())
        for build in (mirror_get_model, ablation_ref.get_model):
            torch.manual_seed(SEED)
            d2, _ = state_digest(build(cfg).state_dict())
            assert d2 == dig, (tag, build.__module__)
        out["models"][tag] = {"kw": kw, "sha256": dig, "tensors": len(sums), "params": sum(p.numel() for p in r.parameters()),
                              "sums": {k: sums[k] for k in list(sums)[:6] + list(sums)[-3:]}}
        print(tag, dig[:16], out["models"][tag]["params"])
    # configs _1_ and _7_ differ only in a ca_type that msrb=False never reads
    torch.manual_seed(SEED)
    d7, _ = state_digest(ref_models.get_model(litehandnet_cfg("X", msrb=False, num_block=[2, 2, 2, 2], ca_type="identity")).state_dict())
    assert d7 == out["models"]["nomsrb"]["sha256"]
    json.dump(out, open(os.path.join(HERE, "init_weights_ablation.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(8)
    ref_models, ref_b, RefLoss, pt, gt, ev = _load_reference()
    for tag in ablation_ref.TAGS:
        model_fixture(tag, ref_models, RefLoss)
    init_fixture(ref_models)
