"""Evaluation twin of train_synthetic.py: a deployed model over synthetic batches, dataset-level PCK / AUC / EPE two ways.

  device : forward -> TopDownEvaluator.update (lhn_heatmap_decode* + ONE lhn_eval_accumulate launch), nothing read back
           inside the loop, compute() once at the end.
  host   : forward -> TopDownDecoder(as_numpy=True).decode (heat maps and predictions copied to the host per batch, as
           the reference does) -> the oracle's numpy keypoint_pck_accuracy / keypoint_auc / keypoint_epe at the end.

    python scripts/eval_synthetic.py [B|A] --batches 50        (LHN_INFER_FUSE=1 in the environment: fused forward)

Prints ONE JSON line: the metrics of both ways, samples per second of each whole loop, the evaluator's share of the device
loop per batch (events on the launch stream: update minus forward) next to the host way's decode + metrics per batch, and
lhn_eval_accumulate alone at N = 13,024 against lhn_pck_accuracy (one of the three metrics, one workgroup) at the same N."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from litehandnet_amd import get_model, heatmap, plan  # noqa: E402
from litehandnet_amd.config import litehandnet_cfg  # noqa: E402
from oracle import heatmap_np as onp  # noqa: E402  (scripts may use the oracle; the package never does)
from train_synthetic import make_batch  # noqa: E402


def kernel_times(dev, N=13024, K=21, reps=20):
    """us per call (events, `reps` calls after 3): lhn_eval_accumulate and lhn_pck_accuracy on the same N x K inputs"""
    g = torch.Generator(device=dev).manual_seed(3)
    gt = torch.rand(N, K, 2, generator=g, device=dev) * 210 + 20
    pred = gt + 6 * torch.randn(N, K, 2, generator=g, device=dev)
    mask = torch.rand(N, K, generator=g, device=dev) > 0.05
    norm = torch.rand(N, 1, generator=g, device=dev).expand(-1, 2).contiguous() * 140 + 60
    st = heatmap._eval_state(K, 20, dev)
    out = {}
    for name, f in (("accumulate", lambda: heatmap._eval_accumulate(st, pred, gt, mask, norm, 0.2, 30.0, 20)),
                    ("pck_accuracy", lambda: heatmap.keypoint_pck_accuracy(pred, gt, mask, 0.2, norm))):
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for a, b in ev:
            a.record()
            f()
            b.record()
        torch.cuda.synchronize()
        t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
        out[name] = dict(median_us=round(t[len(t) // 2], 2), min_us=round(t[0], 2), max_us=round(t[-1], 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("variant_pos", nargs="?", default=None, choices=["A", "B"])
    ap.add_argument("--variant", default="B", choices=["A", "B"])
    ap.add_argument("--batches", type=int, default=50)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--no-host-loop", action="store_true", help="skip the decode-to-numpy + oracle comparison loop")
    args = ap.parse_args()
    variant = args.variant_pos or args.variant
    dev = torch.device("cuda:0")
    cfg = litehandnet_cfg(variant, image_size=args.size)
    torch.manual_seed(0)
    model = get_model(cfg).to(dev).eval()
    model.deploy_model()
    gen = torch.Generator(device=dev).manual_seed(1)
    codes = torch.rand(21, 3, generator=gen, device=dev) * 2 - 1
    n, size, M = args.batch, args.size, args.batches
    data = [make_batch(n, size, gen, dev, codes) for _ in range(M)]
    base = dict(center=torch.full((n, 2), size / 2.0, device=dev), scale=torch.full((n, 2), size / 200.0, device=dev),
                joints_3d_visible=torch.ones(n, 21, 3, device=dev), bbox=torch.tensor([[0.0, 0.0, size, size]]).repeat(n, 1).to(dev),
                bbox_score=torch.ones(n), bbox_id=torch.arange(n), image_file=None)
    metas = [dict(base, joints_3d=j) for _, j in data]
    ev = heatmap.TopDownEvaluator(cfg)
    dec = heatmap.TopDownDecoder(cfg, as_numpy=True)
    with torch.no_grad():
        for img, _ in data[:3]:                              # plans, tables, library load
            ev.update(metas[0], model(img))
        ev.reset()
        torch.cuda.synchronize()

        # ---- device loop
        marks = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(M)]
        t0 = time.perf_counter()
        for (img, _), meta, (e0, e1, e2) in zip(data, metas, marks):
            e0.record()
            out = model(img)
            e1.record()
            ev.update(meta, out)
            e2.record()
        res = ev.compute()                                   # the one read-back
        t_dev = time.perf_counter() - t0
        fwd = sorted(a.elapsed_time(b) for a, b, _ in marks)
        upd = sorted(b.elapsed_time(c) for _, b, c in marks)

        # ---- host loop: what the parent commit offers for the same three numbers
        host = None
        if not args.no_host_loop:
            P, G, t_dec = [], [], 0.0
            t0 = time.perf_counter()
            for (img, j), meta in zip(data, metas):
                out = model(img)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                P.append(dec.decode(meta, out)["preds"][..., :2])
                G.append(j[..., :2].cpu().numpy())
                t_dec += time.perf_counter() - t1
            t1 = time.perf_counter()
            pred, gt = np.concatenate(P), np.concatenate(G)
            mask = np.ones(pred.shape[:2], bool)
            thr = np.full((pred.shape[0], 2), float(size), np.float32)
            hres = [("PCK", float(onp.keypoint_pck_accuracy(pred, gt, mask, ev.pck_thr, thr)[1])),
                    ("AUC", float(onp.keypoint_auc(pred, gt, mask, int(ev.auc_nor), ev.num_step))),
                    ("EPE", float(onp.keypoint_epe(pred, gt, mask)))]
            t_met = time.perf_counter() - t1
            t_host = time.perf_counter() - t0
            host = dict(metrics=dict(hres), samples_per_s=round(n * M / t_host, 1),
                        decode_and_metrics_ms_per_batch=round((t_dec + t_met) * 1e3 / M, 4),
                        decode_ms_per_batch=round(t_dec * 1e3 / M, 4), metrics_ms_total=round(t_met * 1e3, 3))
    med = lambda v: v[len(v) // 2]  # noqa: E731
    line = dict(script="eval_synthetic", variant=variant, deployed=True, infer_fuse=bool(plan.infer_fuse_enabled()),
                batch=n, batches=M, image_size=size, samples=n * M, metrics=dict(res),
                samples_per_s=round(n * M / t_dev, 1),
                forward_ms_per_batch=dict(median=round(med(fwd), 4), min=round(fwd[0], 4), max=round(fwd[-1], 4)),
                evaluator_ms_per_batch=dict(median=round(med(upd), 4), min=round(upd[0], 4), max=round(upd[-1], 4)),
                evaluator_share_of_forward=round(med(upd) / med(fwd), 4), host=host, kernels_n13024_us=kernel_times(dev))
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
