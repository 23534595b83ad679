"""Data and child processes of tests/test_eval_metrics_gpu.py.

    python tests/check_eval_metrics.py stream OUT.npz            one shot / batches of 64 / shuffled batches -> the three states
    python tests/check_eval_metrics.py rank   OUT.npz N          one gloo rank (RANK, WORLD_SIZE, MASTER_* in the environment)

Each mode writes the raw int64 evaluator state(s) and the float64 EPE(s) to OUT.npz; exit code 3 when states that have to
agree do not.  `case2_data` is the seeded dataset-size input of the tests (imported by them)."""
import os
import sys

ROOT = os.environ.get("LHN_REPO") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

K = 21
DEAD_JOINT = 7          # masked in every sample: acc = -1, drops out of the means
PCK_THR, AUC_NOR, NUM_STEP = 0.2, 30, 20


def case2_data(N, seed):
    """gt ~ U(20, 230), pred = gt + N(0, 6) (float32), 5 % of the joints masked at random, one joint masked everywhere, six
    samples with a zero in the PCK normaliser; rows 0..19 sit EXACTLY on AUC threshold i/20 (distance 1.5 i px / 30, strict
    `<`: a miss at threshold i, a hit at i + 1), rows 20..419 within float32 rounding of a threshold (PCK's and AUC's)."""
    r = np.random.default_rng(seed)
    gt = r.uniform(20, 230, (N, K, 2)).astype(np.float32)
    pred = (gt + r.normal(0, 6, (N, K, 2)).astype(np.float32)).astype(np.float32)
    mask = r.random((N, K)) >= 0.05
    mask[:, DEAD_JOINT] = False
    box = r.uniform(60, 200, N).astype(np.float32)
    norm = np.stack([box, box], 1)
    for i in range(20):
        gt[i] = np.floor(gt[i])
        pred[i] = gt[i] + np.array([1.5 * i, 0], np.float32)
    near = np.arange(20, 420)
    step = r.integers(1, NUM_STEP, (len(near), K)).astype(np.float32)
    ang = r.uniform(0, 2 * np.pi, (len(near), K)).astype(np.float32)
    rad = (step * np.float32(AUC_NOR / NUM_STEP)).astype(np.float32)             # AUC: distance / 30 ~ step / 20
    rad[200:] = (np.float32(PCK_THR) * box[near[200:], None]).astype(np.float32)  # PCK: distance / box ~ 0.2
    pred[near] = gt[near] + np.stack([rad * np.cos(ang), rad * np.sin(ang)], -1).astype(np.float32)
    mask[near] = True
    mask[near, DEAD_JOINT] = False
    norm[430:433, 0] = 0
    norm[433:436, 1] = 0
    return pred, gt, mask, norm


def _evaluator():
    from litehandnet_amd import heatmap
    from litehandnet_amd.config import litehandnet_cfg
    return heatmap.TopDownEvaluator(litehandnet_cfg("B"), pck_thr=PCK_THR, auc_nor=AUC_NOR, num_step=NUM_STEP)


def feed(ev, data, order):
    """order: list of index arrays, one per update_preds call"""
    pred, gt, mask, norm = data
    for idx in order:
        ev.update_preds(pred[idx], gt[idx], mask[idx], norm[idx])
    return ev


def orders(N, seed=5):
    b = [np.arange(s, min(s + 64, N)) for s in range(0, N, 64)]
    sh = [b[i] for i in np.random.default_rng(seed).permutation(len(b))]
    return dict(one=[np.arange(N)], batches=b, shuffled=sh)


def raw(ev):
    return ev._st().cpu().numpy().copy()


def main():
    mode, out = sys.argv[1], sys.argv[2]
    import torch
    from litehandnet_amd import _lib
    assert _lib.lib().lhn_deterministic() == int(os.environ.get("LHN_DETERMINISTIC", "0") == "1")
    res, ok = {}, True
    if mode == "stream":
        for N in (2727, 13024):
            data = case2_data(N, N)
            st = {}
            for name, order in orders(N).items():
                ev = feed(_evaluator(), data, order)
                st[name] = raw(ev)
                res[f"state_{N}_{name}"] = st[name]
                res[f"epe_{N}_{name}"] = np.float64(dict(ev.compute())["EPE"])
            ok = ok and np.array_equal(st["one"], st["batches"]) and np.array_equal(st["one"], st["shuffled"])
            ok = ok and res[f"epe_{N}_one"].tobytes() == res[f"epe_{N}_batches"].tobytes() == res[f"epe_{N}_shuffled"].tobytes()
    elif mode == "rank":
        import torch.distributed as dist
        N = int(sys.argv[3])
        rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        try:
            data = case2_data(N, N)
            mine = np.arange(N)[rank::world]                                      # interleaved shards
            ev = feed(_evaluator(), data, [mine[s:s + 64] for s in range(0, len(mine), 64)])
            res["local"] = raw(ev)
            ev.reduce_()
            res["state"] = raw(ev)
            res["metrics"] = np.array([v for _, v in ev.compute()], np.float64)
            dist.barrier()
        finally:
            dist.destroy_process_group()
    else:
        raise SystemExit(f"unknown mode {mode}")
    np.savez(out, **res)
    print("EVAL_CHILD", mode, "ok" if ok else "MISMATCH", flush=True)
    sys.exit(0 if ok else 3)


if __name__ == "__main__":
    main()
