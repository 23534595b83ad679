"""Float64 companions of the model fixtures.  RUNS ONLY IN THE BUILD CONTAINER (needs the reference, see make_golden.py).

The fp32 fixtures (model_<tag>.npz) hold the reference's fp32 results on the host that generated them; fp32 convolutions
and BatchNorm on the CPU round differently with the thread count and instruction set, so on another host the oracle's fp32
result may differ from them by more than the oracle's own error.  This runs the REAL reference in float64 on the same
inputs and weights (train-mode BN, dropout off) and writes model_<tag>_f64.npz: a summary of the heat map
(heatmap_summary), and for the training cases the loss and every parameter's gradient norm.  tests/test_oracle_golden.py
compares the float64 oracle to these tightly and bounds its fp32 comparison by both sides' measured fp32 error.

    python tests/golden/make_golden_f64.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import ROOT, _load_reference, _no_dropout  # noqa: E402

sys.path.insert(0, ROOT)
from litehandnet_amd.config import litehandnet_cfg  # noqa: E402
from oracle import heatmap_np as onp  # noqa: E402
from oracle import synth, torch_ref  # noqa: E402

# tag -> (variant, cfg overrides, with loss + backward); the same cases tests/test_oracle_golden.py runs
CASES = {"B_64": ("B", {}, True), "A_64": ("A", {}, True), "Bca_64": ("B", {"rbu_ca": "ca"}, True),
         "M_128": ("M", {}, True), "Bse_64": ("B", {"msrb_ca": "se", "rbu_ca": "se"}, True),
         "Asilu_64": ("A", {"activation": "silu"}, True), "Mact_128": ("M", {"output_acitivation": True}, True),
         "H1_128": ("H", {"num_stack": 1}, False), "H2_128": ("H", {"num_stack": 2}, False),
         "L18_128": ("L", {"depth": 18}, False)}
HEATMAP_SAMPLE = 8192


def projection(numel):
    """The fixed weights of heatmap_proj: w . heat map checks every element of a map that is not stored whole."""
    return np.random.default_rng(0).standard_normal(numel)


def heatmap_summary(y64, y32):
    """What the test needs of the float64 heat map (the whole map would make these files too large): a fixed seeded sample
    of HEATMAP_SAMPLE elements, its projection on projection(), its peak and the fp32 fixture's largest error."""
    flat = y64.reshape(-1)
    idx = np.sort(np.random.default_rng(1).choice(flat.size, HEATMAP_SAMPLE, replace=False))
    return {"heatmap_idx": idx, "heatmap_sample": flat[idx], "heatmap_proj": np.float64(flat @ projection(flat.size)),
            "heatmap_absmax": np.float64(np.abs(flat).max()), "heatmap_f32_err": np.float64(np.abs(y32 - y64).max())}


def main():
    torch.set_num_threads(8)
    ref_models, ref_b, RefLoss, _, _, _ = _load_reference()
    loss_fn = RefLoss(litehandnet_cfg("A"))          # the loss the fp32 training fixtures were made with
    for tag, (variant, kw, train) in CASES.items():
        g = np.load(os.path.join(HERE, f"model_{tag}.npz"))
        n, size, seed = int(g["n"]), int(g["size"]), int(g["seed"])
        cfg = litehandnet_cfg(variant, **kw)
        r = ref_b.LiteHandNet(cfg) if variant == "B" else ref_models.get_model(cfg)
        r.load_state_dict(synth.synth_state_dict(r, seed))
        r = r.double().train()
        _no_dropout(r)
        y = r(synth.synth_images(n, size, seed).double())
        out = heatmap_summary(y.detach().numpy(), g["heatmap"])
        if train:
            hs = size // 4
            j = synth.synth_joints(n, 21, size, seed + 1)
            tgt = np.stack([onp.msra_generate_target(a, np.ones_like(a), [size, size], [hs, hs])[0] for a in j])
            meta = {"target": torch.from_numpy(tgt).double(), "target_weight": torch.from_numpy(g["target_weight"]).double()}
            loss, _ = loss_fn(y, meta)
            loss.backward()
            keys = sorted(k for k, _ in r.named_parameters())
            assert keys == g["grad_keys"].tolist()
            gn = dict((k, float(p.grad.norm())) for k, p in r.named_parameters())
            out.update(loss=np.float64(float(loss.detach())), grad_keys=np.array(keys), grad_norms=np.array([gn[k] for k in keys], np.float64))
        # the oracle in float64 on the same case (what the test asserts, printed here for the record)
        o = torch_ref.get_model(cfg)
        o.load_state_dict(synth.synth_state_dict(o, seed))
        o = o.double().train()
        _no_dropout(o)
        yo = o(synth.synth_images(n, size, seed).double()).detach().numpy()
        scale = float(out["heatmap_absmax"])
        print(f"[{tag}] float64 oracle vs reference: heat map {np.abs(yo - y.detach().numpy()).max() / scale:.2e}; "
              f"fp32 fixture vs float64 reference {float(out['heatmap_f32_err']) / scale:.2e}")
        np.savez_compressed(os.path.join(HERE, f"model_{tag}_f64.npz"), **out)


if __name__ == "__main__":
    main()
