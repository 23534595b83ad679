"""Training-step time of a model at another width than 128: `python scripts/bench_width256.py [A|M|X] [bs] [steps] [channels]`
(defaults A, 64, 10, 256; the reference's configs use 128, 160 and 256).  bench.py's loop (Trainer.step on synthetic images and targets
at 256 x 256, dropout on); events on the launch stream after 3 warm-up steps.  Under `rocprofv3 --kernel-trace`
scripts/prof_kernels.py reads the per-kernel durations."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from litehandnet_amd import get_loss, get_model
from litehandnet_amd.config import litehandnet_cfg
from litehandnet_amd.train import Trainer
variant = sys.argv[1] if len(sys.argv) > 1 else "A"
bs = int(sys.argv[2]) if len(sys.argv) > 2 else 64
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
channels = int(sys.argv[4]) if len(sys.argv) > 4 else 256
dev = torch.device("cuda:0")
cfg = litehandnet_cfg(variant, channels=channels)
m = get_model(cfg).to(dev).train()
tr = Trainer(m, get_loss(cfg), lr=5e-4, world_size=1)
g = torch.Generator(device=dev).manual_seed(3)
x = torch.randn(bs, 3, 256, 256, device=dev, generator=g)
meta = {"target": torch.rand(bs, 21, 64, 64, device=dev, generator=g), "target_weight": torch.ones(bs, 21, 1, device=dev)}
for _ in range(3):
    loss = tr.step(x, meta)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(steps):
    loss = tr.step(x, meta)
e1.record(); torch.cuda.synchronize()
print(f"{variant} channels={channels} bs{bs}: step_ms {e0.elapsed_time(e1) / steps:.3f} loss {float(loss.detach()):.5f}", flush=True)
