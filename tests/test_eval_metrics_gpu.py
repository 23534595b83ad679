"""GPU: dataset-level PCK / AUC / EPE (lhn_eval_accumulate / lhn_eval_finalize, heatmap.keypoint_auc / keypoint_epe /
TopDownEvaluator) against oracle/heatmap_np.py and the reference-written fixture tests/golden/decode.npz.

Bars.  Counts (valid_*, hit_*, epe_cnt) are integers: compared EXACTLY with the counts formed from the oracle's own
_calc_distances (`d != -1`, `d < thr`); acc[K], cnt and each threshold's mean accuracy follow from them and are exact too.
PCK and AUC (float64 means of those ratios): abs <= 1e-12, the bar tests/test_oracle_golden.py holds the oracle to (the
order of the last additions is free).  EPE: relative <= 1e-6: the reference returns a float32 pairwise sum / count, the
device an exact fixed-point sum of the same float32 distances; the reference sits 3.8e-8 (N = 6) to 1.1e-7 (N = 13,024) from
the float64 mean of those distances, so 1e-6 (~8 float32 ulp) leaves a factor 9.  The fixed-point words themselves are
compared exactly with the same sum formed from the oracle's float32 distances (whole pixels + fractions rounded to 2^-32)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from check_eval_metrics import AUC_NOR, DEAD_JOINT, K, NUM_STEP, PCK_THR, case2_data, feed, orders, raw, _evaluator
from litehandnet_amd import get_model, heatmap, plan
from litehandnet_amd.config import litehandnet_cfg
from oracle import heatmap_np as onp
from oracle import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "check_eval_metrics.py")
ABS_MEAN, REL_EPE = 1e-12, 1e-6


def _oracle_state(pred, gt, mask, norm, pck_thr=PCK_THR, auc_nor=AUC_NOR, num_step=NUM_STEP):
    """The evaluator's state from the oracle's own distances, plus each threshold's mean accuracy."""
    N = pred.shape[0]
    d = onp._calc_distances(pred, gt, mask, norm)                                  # [K, N] float32, -1 = dropped
    v = d != -1
    st = dict(valid_pck=v.sum(1), hit_pck=((d < pck_thr) & v).sum(1))
    da = onp._calc_distances(pred, gt, mask, np.tile(np.array([[auc_nor, auc_nor]]), (N, 1)))
    va = da != -1
    st["valid_auc"] = va.sum(1)
    st["hit_auc"] = np.stack([((da < i / num_step) & va).sum(1) for i in range(num_step)])
    de = onp._calc_distances(pred, gt, mask, np.ones((N, 2), np.float32))
    e = de[de != -1].astype(np.float64)
    st["epe_cnt"] = int(e.size)
    st["epe_hi"] = int(np.floor(e).sum())
    st["epe_lo"] = int(np.rint((e - np.floor(e)) * 4294967296.0).astype(np.int64).sum())
    st["epe_bad"] = 0
    avg = [onp.keypoint_pck_accuracy(pred, gt, mask, i / num_step, np.tile(np.array([[auc_nor, auc_nor]]), (N, 1)))[1]
           for i in range(num_step)]
    return st, np.array(avg, np.float64)


def _check_state(got, want):
    for k in ("valid_pck", "hit_pck", "valid_auc", "hit_auc"):
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    for k in ("epe_cnt", "epe_hi", "epe_lo", "epe_bad"):
        assert got[k] == want[k], (k, got[k], want[k])


def _check_metrics(ev, pred, gt, mask, norm, tag):
    """state, per-joint PCK, PCK, AUC, EPE of evaluator `ev` against the oracle on the concatenated inputs"""
    want, avg = _oracle_state(pred, gt, mask, norm, ev.pck_thr, int(ev.auc_nor), ev.num_step)
    got = ev.state()
    _check_state(got, want)
    with np.errstate(divide="ignore", invalid="ignore"):
        thr_avg = np.array([(h[want["valid_auc"] > 0] / got["valid_auc"][want["valid_auc"] > 0]).mean() for h in got["hit_auc"]])
    assert np.array_equal(thr_avg, avg)                                           # each threshold's mean accuracy: exact
    acc, pck, cnt = onp.keypoint_pck_accuracy(pred, gt, mask, ev.pck_thr, norm)
    auc = onp.keypoint_auc(pred, gt, mask, int(ev.auc_nor), ev.num_step)
    epe = float(onp.keypoint_epe(pred, gt, mask))
    o = ev._final()
    m = dict(ev.compute())
    print(f"{tag}: PCK {m['PCK']!r} oracle {float(pck)!r} | AUC {m['AUC']!r} oracle {auc!r} | EPE {m['EPE']!r} oracle {epe!r} "
          f"rel {abs(m['EPE'] - epe) / max(epe, 1e-30):.3e} | cnt {int(o[ev.num_joints + 1])}")
    assert list(m) == ["PCK", "AUC", "EPE"]
    assert np.array_equal(ev.per_joint_pck(), np.asarray(acc, np.float64))        # ratios of equal integers: exact
    assert int(o[ev.num_joints + 1]) == cnt
    assert abs(m["PCK"] - float(pck)) <= ABS_MEAN
    assert abs(m["AUC"] - auc) <= ABS_MEAN
    assert abs(m["EPE"] - epe) <= REL_EPE * abs(epe)
    return m


def test_fixture_auc_epe(dev, golden_dir):
    """Case 1: keypoint_auc / keypoint_epe on decode.npz against the numbers the REFERENCE stored in it."""
    g = np.load(os.path.join(golden_dir, "decode.npz"))
    auc = heatmap.keypoint_auc(g["preds"], g["gt"], g["mask"], 30)
    epe = heatmap.keypoint_epe(g["preds"], g["gt"], g["mask"])
    print(f"fixture: AUC {auc!r} stored {float(g['auc'])!r} | EPE {epe!r} stored {float(g['epe'])!r}")
    assert isinstance(auc, float) and isinstance(epe, float)
    assert abs(auc - float(g["auc"])) <= ABS_MEAN
    assert abs(epe - float(g["epe"])) <= REL_EPE * abs(float(g["epe"]))
    assert abs(auc - onp.keypoint_auc(g["preds"], g["gt"], g["mask"], 30)) <= ABS_MEAN
    # and the device tensors route, num_step other than 20
    auc7 = heatmap.keypoint_auc(torch.from_numpy(g["preds"]).to(dev), torch.from_numpy(g["gt"]).to(dev),
                                torch.from_numpy(g["mask"]).to(dev), 30, num_step=7)
    assert abs(auc7 - onp.keypoint_auc(g["preds"], g["gt"], g["mask"], 30, 7)) <= ABS_MEAN


@pytest.mark.parametrize("N", [2727, 13024])
def test_dataset_size(dev, N):
    """Case 2: dataset-size inputs in one shot, with masked joints, dropped samples and on-threshold rows."""
    pred, gt, mask, norm = case2_data(N, N)
    ev = feed(_evaluator(), (pred, gt, mask, norm), [np.arange(N)])
    m = _check_metrics(ev, pred, gt, mask, norm, f"dataset_{N}")
    assert ev.per_joint_pck()[DEAD_JOINT] == -1.0
    live = np.arange(K) != DEAD_JOINT
    assert (np.diff(ev.state()["hit_auc"][:, live], axis=0) > 0).all() and 0.5 < m["AUC"] < 0.9    # every threshold populated
    # the on-threshold rows alone: distance == float32(i / 20) exactly -> a miss at threshold i, a hit from i + 1 on
    on = np.arange(20)
    e2 = feed(_evaluator(), (pred, gt, mask, norm), [on])
    s = e2.state()
    for k in range(K):
        want = np.array([sum(1 for i in on if mask[i, k] and i < t) for t in range(NUM_STEP)])
        assert np.array_equal(s["hit_auc"][:, k], want), (k, s["hit_auc"][:, k], want)
    _check_metrics(e2, pred[on], gt[on], mask[on], norm[on], f"on_threshold_{N}")
    near = np.arange(20, 420)
    _check_metrics(feed(_evaluator(), (pred, gt, mask, norm), [near]), pred[near], gt[near], mask[near], norm[near],
                   f"near_threshold_{N}")
    # keypoint_auc / keypoint_epe at this size
    assert abs(heatmap.keypoint_auc(pred, gt, mask, AUC_NOR) - onp.keypoint_auc(pred, gt, mask, AUC_NOR)) <= ABS_MEAN
    epe = float(onp.keypoint_epe(pred, gt, mask))
    assert abs(heatmap.keypoint_epe(pred, gt, mask) - epe) <= REL_EPE * epe


@pytest.mark.parametrize("N", [2727, 13024])
def test_streaming_equals_one_shot(dev, N):
    """Case 3, default mode: batches of 64 (ragged tail), one batch, shuffled batches -> the same state words, EPE within
    its bar (it is in fact the same double: the sum is fixed point)."""
    data = case2_data(N, N)
    st, epe = {}, {}
    for name, order in orders(N).items():
        ev = feed(_evaluator(), data, order)
        st[name], epe[name] = raw(ev), dict(ev.compute())["EPE"]
    assert N % 64 != 0 and len(orders(N)["batches"]) == -(-N // 64)
    assert np.array_equal(st["one"], st["batches"]) and np.array_equal(st["one"], st["shuffled"])
    for name in ("batches", "shuffled"):
        assert abs(epe[name] - epe["one"]) <= REL_EPE * abs(epe["one"])
    ev.reset()
    assert not raw(ev).any()


def test_streaming_deterministic_mode(dev, tmp_path):
    """Case 3 under LHN_DETERMINISTIC=1 (fresh child, own time limit): the three feeds give identical states and bit-equal EPE
    (the child exits 3 otherwise), and they are the states of this (default-mode) process."""
    out = str(tmp_path / "stream.npz")
    env = dict(os.environ, LHN_DETERMINISTIC="1", LHN_REPO=ROOT)
    r = subprocess.run([sys.executable, CHILD, "stream", out], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    z = np.load(out)
    for N in (2727, 13024):
        data = case2_data(N, N)
        ev = feed(_evaluator(), data, orders(N)["batches"])
        for name in ("one", "batches", "shuffled"):
            assert np.array_equal(z[f"state_{N}_{name}"], raw(ev)), (N, name)
            assert z[f"epe_{N}_{name}"].tobytes() == z[f"epe_{N}_one"].tobytes()
        assert float(z[f"epe_{N}_one"]) == dict(ev.compute())["EPE"]


def _meta(n, size, seed):
    r = np.random.default_rng(seed)
    j = np.zeros((n, K, 3), np.float32)
    j[..., :2] = r.uniform(4, size - 4, (n, K, 2))
    v = np.ones((n, K, 3), np.float32)
    v[r.random((n, K)) < 0.15] = 0
    wh = r.uniform(0.6 * size, size, (n, 2)).astype(np.float32)
    bbox = np.concatenate([r.uniform(0, 4, (n, 2)).astype(np.float32), wh], 1)
    center = (bbox[:, :2] + wh / 2).astype(np.float32)
    scale = (np.stack([wh.max(1), wh.max(1)], 1) / 200.0 * 1.25).astype(np.float32)
    return dict(joints_3d=torch.from_numpy(j), joints_3d_visible=torch.from_numpy(v), bbox=torch.from_numpy(bbox),
                center=torch.from_numpy(center), scale=torch.from_numpy(scale), bbox_score=torch.ones(n),
                bbox_id=torch.arange(n) + 100 * seed, image_file=[f"img_{seed}_{i}.jpg" for i in range(n)])


@pytest.fixture(scope="module")
def deployed_b(dev):
    cfg = litehandnet_cfg("B", image_size=64)
    cfg.MODEL["ca_dropout"] = 0.0
    m = get_model(cfg)
    m.load_state_dict(synth.synth_state_dict(m, 21))
    m.to(dev).eval()
    m.deploy_model()
    xs = [synth.synth_images(4, 64, 50 + b).to(dev) for b in range(3)]
    with torch.no_grad():
        outs = [m(x).clone() for x in xs]
    plan.set_infer_fuse(None)
    return outs


@pytest.mark.parametrize("mode", ["default", "unbiased", "udp"])
def test_evaluator_end_to_end(dev, deployed_b, mode):
    """Case 4: deployed variant B, 3 batches: update x 3 + compute against TopDownDecoder(as_numpy=True).decode results
    concatenated and pushed through the oracle's metrics (both sides decode with the same device kernels)."""
    cfg = litehandnet_cfg("B", image_size=64)
    cfg.PIPELINE["unbiased_encoding"] = mode == "unbiased"
    cfg.PIPELINE["use_udp"] = mode == "udp"
    ev = heatmap.TopDownEvaluator(cfg)
    dec = heatmap.TopDownDecoder(cfg, as_numpy=True)
    assert ev.decoder.post_process == dec.post_process and ev.decoder.use_udp == dec.use_udp and ev.decoder.kernel == dec.kernel
    P, G, M, T = [], [], [], []
    for b, out in enumerate(deployed_b):
        meta = _meta(out.shape[0], 64, 7 + b)
        ev.update(meta, out)
        res = dec.decode(meta, out)
        P.append(res["preds"][..., :2])
        G.append(meta["joints_3d"].numpy()[..., :2])
        M.append(meta["joints_3d_visible"].numpy()[..., 0] > 0)
        thr = meta["bbox"].numpy()[:, 2:].max(1)
        T.append(np.stack([thr, thr], 1))
    pred, gt, mask, norm = (np.concatenate(a) for a in (P, G, M, T))
    assert np.isfinite(pred).all()
    _check_metrics(ev, pred.astype(np.float32), gt, mask, norm.astype(np.float32), f"end_to_end_{mode}")
    # the device-side meta route and a metric subset
    ev2 = heatmap.TopDownEvaluator(cfg, metrics=["EPE", "PCK"])
    for b, out in enumerate(deployed_b):
        meta = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in _meta(out.shape[0], 64, 7 + b).items()}
        ev2.update(meta, out)
    assert np.array_equal(raw(ev2), raw(ev))
    assert [k for k, _ in ev2.compute()] == ["PCK", "EPE"]


def test_update_does_not_synchronise(dev, deployed_b):
    """Case 5: update / update_preds under torch's sync debug mode 'error': an .item(), .cpu() or synchronize inside raises."""
    cfg = litehandnet_cfg("B", image_size=64)
    ev = heatmap.TopDownEvaluator(cfg)
    metas = [_meta(o.shape[0], 64, 7 + b) for b, o in enumerate(deployed_b)]
    pred, gt, mask, norm = case2_data(500, 3)
    ev.update(metas[0], deployed_b[0])                       # first call: library load, state allocation
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):                    # the mode is live: a read-back raises
            deployed_b[0].sum().item()
        for meta, out in zip(metas[1:], deployed_b[1:]):
            ev.update(meta, out)
        ev.update_preds(pred, gt, mask, norm)
        ev.update_preds(torch.from_numpy(pred).to(dev, non_blocking=True), gt, mask, norm[:, 0])
    finally:
        torch.cuda.set_sync_debug_mode(old)
    assert ev.state()["epe_cnt"] > 0


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_ranks_reduce(dev, tmp_path):
    """Case 6: two fresh child processes sharing cuda:0 over gloo, half of the N = 2,727 data each: after reduce_ both hold the
    single-process state exactly, hence the single-process metrics."""
    N = 2727
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), WORLD_SIZE="2", LHN_REPO=ROOT,
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    outs = [str(tmp_path / f"rank{r}.npz") for r in range(2)]
    procs = [subprocess.Popen([sys.executable, CHILD, "rank", outs[r], str(N)], env=dict(env, RANK=str(r)), cwd=ROOT,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    logs, codes = [], []
    try:
        for p in procs:
            try:
                logs.append(p.communicate(timeout=300)[0])
            except subprocess.TimeoutExpired:
                logs.append("timeout")
            codes.append(p.poll())
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    assert codes == [0, 0], (codes, [l[-2000:] for l in logs])
    data = case2_data(N, N)
    single = feed(_evaluator(), data, [np.arange(N)])
    want, m = raw(single), np.array([v for _, v in single.compute()])
    for r in range(2):
        z = np.load(outs[r])
        assert not np.array_equal(z["local"], want)
        assert np.array_equal(z["state"], want), r
        assert np.array_equal(z["metrics"][:2], m[:2]) and abs(z["metrics"][2] - m[2]) <= REL_EPE * m[2]
    assert np.array_equal(np.load(outs[0])["local"] + np.load(outs[1])["local"], want)
    # without a process group reduce_ leaves the state alone
    assert np.array_equal(raw(single.reduce_()), want)
