"""Child process of tests/test_fwd_fin_step_gpu.py: one training step on seeded inputs; loss, output, every gradient (and all of them
as one flat vector) and every buffer written to an .npz.  LHN_FWD_FIN_CONSUMER and LHN_DETERMINISTIC are read once per process, hence
the child.

    python tests/fwd_fin_child.py block OUT.npz     MSRB(128) -> RepBasicUnit(128), batch 2, 64 x 64 map
    python tests/fwd_fin_child.py B OUT.npz         variant B, batch 2, 64 x 64 input"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from litehandnet_amd import get_loss, get_model  # noqa: E402
from litehandnet_amd.config import litehandnet_cfg  # noqa: E402
from litehandnet_amd.engine import PlanModule  # noqa: E402
from litehandnet_amd.litehourglass import MSRB, RepBasicUnit  # noqa: E402
from oracle import synth  # noqa: E402


class Block(PlanModule):
    def __init__(self):
        super().__init__()
        self.msrb = MSRB(128, 128, "ca", p_drop=0.0)
        self.unit = RepBasicUnit(128, 128, "ca", p_drop=0.0)

    def emit(self, pb, x, out=None):
        return self.unit.emit(pb, self.msrb.emit(pb, x), out=out)


dev = torch.device("cuda:0")
which, dst = sys.argv[1], sys.argv[2]
if which == "block":
    m = Block()
    x = torch.randn(2, 128, 64, 64, generator=torch.Generator().manual_seed(7)).to(dev).requires_grad_()
    t = torch.randn(2, 128, 64, 64, generator=torch.Generator().manual_seed(3)).to(dev)
else:
    cfg = litehandnet_cfg("B")
    cfg.MODEL["ca_dropout"] = 0.0
    crit = get_loss(cfg)
    m = get_model(cfg)
    x = synth.synth_images(2, 64, 7).to(dev)
    t = torch.rand(2, 21, 16, 16, generator=torch.Generator().manual_seed(3)).to(dev)
m.load_state_dict({k: v.clone() for k, v in synth.synth_state_dict(m, 5).items()})
m.to(dev).train()
y = m(x)
if which == "block":
    loss = ((y - t) ** 2).mean()
else:
    loss, _ = crit(y, {"target": t, "target_weight": torch.ones(2, 21, 1, device=dev)})
m.zero_grad()
loss.backward()
out = {"loss": np.float64(float(loss)), "y": y.detach().cpu().numpy()}
if which == "block":
    out["dx"] = x.grad.detach().cpu().numpy()
flat = []
for k, p in m.named_parameters():
    out[f"g.{k}"] = p.grad.detach().cpu().numpy()
    flat.append(out[f"g.{k}"].reshape(-1))
out["gflat"] = np.concatenate(flat)
for k, b in m.named_buffers():
    out[f"b.{k}"] = b.detach().cpu().numpy()
np.savez(dst, **out)
