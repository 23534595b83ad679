"""Train-step time of one `hourglass_ablation` network (recorded in DESIGN.md section 5.2, not gated anywhere):

    python scripts/bench_ablation.py TAG [--batch 64] [--size 224] [--steps 20] [--warmup 5]

TAG is one of ca, se, 1x1, identity, cbam, nomsrb, rca.  Prints one JSON line: ms per training step (forward + loss +
backward + Adam through litehandnet_amd.train.Trainer, CUDA events around `steps` steps) and, measured in the same process,
the device-to-device copy rate of a 1 GiB buffer (the yardstick for the bytes a streaming kernel must move).  The cost of an
attention is the difference between its TAG and `identity`, from alternating fresh processes."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from litehandnet_amd import get_loss, get_model  # noqa: E402
from litehandnet_amd.config import litehandnet_cfg  # noqa: E402
from litehandnet_amd.train import Trainer  # noqa: E402

KW = {"ca": {}, "se": dict(ca_type="se"), "1x1": dict(ca_type="1x1"), "identity": dict(ca_type="identity"), "cbam": dict(ca_type="cbam"),
      "nomsrb": dict(msrb=False, num_block=[2, 2, 2, 2]), "rca": dict(rca=True)}


def _timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("tag", choices=sorted(KW))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = litehandnet_cfg("X", image_size=a.size, **KW[a.tag])
    torch.manual_seed(0)
    model = get_model(cfg).to(dev).train()
    tr = Trainer(model, get_loss(cfg))
    img = torch.randn(a.batch, 3, a.size, a.size, device=dev)
    meta = {"target": torch.rand(a.batch, 21, a.size // 4, a.size // 4, device=dev), "target_weight": torch.ones(a.batch, 21, 1, device=dev)}
    for _ in range(a.warmup):
        tr.step(img, meta)
    torch.cuda.synchronize()
    step_ms = _timed(lambda: tr.step(img, meta), a.steps)
    src = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    dst = torch.empty_like(src)
    dst.copy_(src)
    copy_ms = _timed(lambda: dst.copy_(src), 10)
    print(json.dumps({"tag": a.tag, "batch": a.batch, "size": a.size, "step_ms": round(step_ms, 3),
                      "copy_TBps": round(2 * src.numel() * 4 / copy_ms / 1e9, 3)}), flush=True)


if __name__ == "__main__":
    main()
