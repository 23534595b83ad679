"""CPU side of tests/test_zz_bench_config_gpu.py, run as a CHILD PROCESS (never touches the GPU): the float64 oracle (arbiter) and
the fp32 oracle (yardstick = what the reference computes on the CPU) of bench.py's workload -- batch 64, 256x256, train-mode
BatchNorm, Dropout2d p = 0.3 with seeded masks where the model has attention modules -- forward + TopdownHeatmapLoss +
backward, for variants B, A, H (stacked hourglass: the target and its weights expanded over the stack axis) and L.  It keeps
what the test compares: the outputs, the loss, the FULL gradient of every parameter in both precisions (`g32_<i>`, `g64_<i>`
in `keys` order, next to their norms `g32` / `g64`) and every running_mean / running_var after the step (`stat32_<name>`,
`stat64_<name>`, names in `stat_keys`).  conftest.py starts it at the beginning of a GPU session so that it runs UNDER the
other GPU tests instead of adding to the suite's wall time; it holds one variant at a time.  A second fp32 step in
channels_last (`g32cl_<i>`, its own process: `channels_last_rc` = its exit status) gives the test a second summation order.
Measured on an 8-core host at 4 threads (the GPU host runs 8), both fp32 runs included: B 47 s / 19 GB peak RSS, A 59 s /
18 GB, H 113 s / 27 GB, L 58 s / 28 GB -- under 5 minutes in all, written in that order (B first: its test runs first and
waits on it).

    python tests/bench_config_oracle.py OUTDIR [B A H L]  ->  OUTDIR/bench_oracle_<variant>.npz (written atomically)
"""
import copy
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from litehandnet_amd import get_model  # noqa: E402
from litehandnet_amd.config import litehandnet_cfg  # noqa: E402
from litehandnet_amd.plan import PlanBuilder  # noqa: E402
from oracle import heatmap_np as onp  # noqa: E402
from oracle import synth, torch_ref  # noqa: E402

P, N, SIZE, SEED = 0.3, 64, 256, 7


def draw_masks(cfg, n, seed, p=P):
    """The masks tests/test_dropout_gpu.py::_attach draws: one [n, C] tensor per attention module in the PLAN's order (the order
    its launch records list them), generator PCG64([seed, index]).  The plan is built on the CPU (no library call)."""
    m = get_model(cfg)
    tensors = list(m.state_dict(keep_vars=True).values())
    pb = PlanBuilder(n, {id(t): j for j, t in enumerate(tensors)}, image_hw=(SIZE, SIZE), with_backward=True, p_drop=p)
    m.emit(pb, pb.image())
    names = {id(mod): k for k, mod in m.named_modules()}
    masks = {}
    for r in pb.recs:
        if r.get("mask") is not None:
            mod = r.get("ca", r.get("att"))
            k = names[id(mod)]
            if k not in masks:
                g = np.random.Generator(np.random.PCG64([seed, len(masks)]))
                masks[k] = torch.from_numpy(((g.random((n, r["y"].C)) < 1 - p) / (1 - p)).astype(np.float32))
    return masks


def _stats(model):
    """{state-dict name: running_mean / running_var} of every BatchNorm, after the step."""
    return {k: v.detach().double().numpy() for k, v in model.state_dict().items() if k.endswith(("running_mean", "running_var"))}


def _setup(variant):
    cfg = litehandnet_cfg(variant)
    ref = torch_ref.get_model(cfg, p_drop=P)
    ref.load_state_dict(synth.synth_state_dict(ref, SEED))
    ref.train()
    masks = draw_masks(cfg, N, SEED + 500)
    x = synth.synth_images(N, SIZE, SEED)
    j = synth.synth_joints(N, 21, SIZE, SEED + 1)
    tgt = torch.from_numpy(np.stack([onp.msra_generate_target(a, np.ones_like(a), [SIZE, SIZE], [64, 64])[0] for a in j]))
    torch_ref.install_masks(ref, masks)
    return cfg, ref, masks, x, tgt, torch.ones(N, 21, 1)


def _loss(cfg, y, tgt, tw):
    if y.dim() == 5:         # stacked hourglass [N, S, K, H, W]: every stack supervised by the same target (see loss.py)
        S = y.shape[1]
        tgt, tw = tgt.unsqueeze(1).expand(-1, S, -1, -1, -1), tw.unsqueeze(1).expand(-1, S, -1, -1)
    return cfg.LOSS.loss_weight[0] * torch_ref.distance_loss(y, tgt.to(y.dtype), tw.to(y.dtype))


def channels_last_grads(variant, path):
    """The same fp32 step in channels_last (another summation order of every convolution): gradients to `path`.  Run in a
    process of its own: torch's CPU channels_last backward corrupts its heap on variant A's stem (a crash there must not take
    the oracle down; the test then has the NCHW run alone for A)."""
    cfg, ref, _, x, tgt, tw = _setup(variant)
    ref = ref.to(memory_format=torch.channels_last)
    _loss(cfg, ref(x.contiguous(memory_format=torch.channels_last)), tgt, tw).backward()
    np.savez(path, **{f"g32cl_{i}": p.grad.contiguous().numpy() for i, (_, p) in enumerate(ref.named_parameters())})


def run(variant, outdir):
    cl = os.path.join(outdir, f"channels_last_{variant}.npz")
    rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--channels-last", cl, variant]).returncode
    G32cl = dict(np.load(cl)) if rc == 0 else {}
    print(f"channels_last fp32 run of {variant}: rc {rc}", flush=True)
    cfg, ref, masks, x, tgt, tw = _setup(variant)
    ref32 = copy.deepcopy(ref)
    y32 = ref32(x)
    l32 = _loss(cfg, y32, tgt, tw)
    l32.backward()
    keys = [k for k, _ in ref32.named_parameters()]
    G32 = [p.grad.contiguous().numpy().astype(np.float32) for _, p in ref32.named_parameters()]
    g32 = np.array([float(p.grad.norm()) for _, p in ref32.named_parameters()])
    s32 = _stats(ref32)
    y32 = y32.detach().numpy()
    del ref32
    ref = ref.double()
    y64 = ref(x.double())
    l64 = _loss(cfg, y64, tgt, tw)
    l64.backward()
    G64 = [p.grad.numpy() for _, p in ref.named_parameters()]
    g64 = np.array([float(p.grad.norm()) for _, p in ref.named_parameters()])
    s64 = _stats(ref)
    tmp = os.path.join(outdir, f"bench_oracle_{variant}.tmp.npz")
    np.savez(tmp, y64=y64.detach().numpy(), y32=y32, l64=float(l64), l32=float(l32), keys=np.array(keys), g64=g64, g32=g32,
             mask_names=np.array(list(masks)), **{f"mask_{i}": v.numpy() for i, v in enumerate(masks.values())},
             **{f"g32_{i}": v for i, v in enumerate(G32)}, **G32cl, channels_last_rc=rc,
             **{f"g64_{i}": v for i, v in enumerate(G64)},
             stat_keys=np.array(list(s64)), **{f"stat32_{k}": v for k, v in s32.items()}, **{f"stat64_{k}": v for k, v in s64.items()})
    os.replace(tmp, os.path.join(outdir, f"bench_oracle_{variant}.npz"))
    print("done", variant, flush=True)


if __name__ == "__main__":
    torch.set_num_threads(max(1, min(8, (os.cpu_count() or 8) // 2)))
    if sys.argv[1] == "--channels-last":
        channels_last_grads(sys.argv[3], sys.argv[2])
        sys.exit(0)
    out = sys.argv[1]
    os.makedirs(out, exist_ok=True)
    for v in (sys.argv[2:] or ["B", "A", "H", "L"]):
        run(v, out)
