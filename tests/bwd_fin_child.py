"""Child process of tests/test_bwd_fin_consumer_gpu.py: one training step of variant B (batch 2, 64 x 64 input) on seeded inputs;
loss, every gradient (and all of them as one flat vector) and every buffer written to an .npz.  LHN_BWD_FIN_CONSUMER and
LHN_DETERMINISTIC are read once per process, hence the child.

    python tests/bwd_fin_child.py OUT.npz"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from litehandnet_amd import get_loss, get_model  # noqa: E402
from litehandnet_amd.config import litehandnet_cfg  # noqa: E402
from oracle import synth  # noqa: E402

dev = torch.device("cuda:0")
cfg = litehandnet_cfg("B")
cfg.MODEL["ca_dropout"] = 0.0
crit = get_loss(cfg)
m = get_model(cfg)
m.load_state_dict({k: v.clone() for k, v in synth.synth_state_dict(m, 5).items()})
m.to(dev).train()
x = synth.synth_images(2, 64, 7).to(dev)
t = torch.rand(2, 21, 16, 16, generator=torch.Generator().manual_seed(3)).to(dev)
meta = {"target": t, "target_weight": torch.ones(2, 21, 1, device=dev)}
y = m(x)
loss, _ = crit(y, meta)
m.zero_grad()
loss.backward()
out = {"loss": np.float64(float(loss)), "y": y.detach().cpu().numpy()}
flat = []
for k, p in m.named_parameters():
    out[f"g.{k}"] = p.grad.detach().cpu().numpy()
    flat.append(out[f"g.{k}"].reshape(-1))
out["gflat"] = np.concatenate(flat)
for k, b in m.named_buffers():
    out[f"b.{k}"] = b.detach().cpu().numpy()
np.savez(sys.argv[1], **out)
