"""Direct C-ABI checks of the fused 3x3 depthwise backward (dgrad + wgrad with its fusions: dx accumulate, gradient addends,
BatchNorm-backward sums of the producer, gated x / y, pooled-attention gradient, parity sub-lattices, the direct dilation-2
path, channel tails, weight-gradient replicas) against a float64 torch reference, at the benchmark shape, at 128 x 128 and on
small maps; the tile kernel it replaced (LHN_DW_BWD_V1=1) must agree, and deterministic mode must repeat its bits."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dw_bwd_cases as dc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 2e-5          # relative to the largest magnitude of each output (float32 sums of <= 8k products vs float64)


def _close(a, b, what):
    scale = max(float(np.abs(b).max()), 1e-30)
    err = float(np.abs(a.astype(np.float64) - b).max()) / scale
    assert err <= TOL, f"{what}: max rel err {err:.3e}"


def _child(tmp_path, env_extra, names, reps):
    out = str(tmp_path / "out.npz")
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, os.path.join(HERE, "dw_bwd_cases.py"), out, str(reps)] + names, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return dict(np.load(out))


@pytest.mark.parametrize("name", list(dc.CASES))
def test_dw_bwd_matches_float64(dev, name):
    g = dc.inputs(name)
    got, ref = dc.run(name, dev, g), dc.reference(name, g)
    for k in ref:
        _close(got[k], ref[k], f"{name} {k}")
    _, _, _, cs, coff, c, _, _ = dc.CASES[name]
    if cs > c:        # channels outside the view are untouched
        before = (g["prior"].numpy() if "prior" in g else np.full(g["x"].shape, 7.0, np.float32))
        np.testing.assert_array_equal(got["dx_outside"], np.concatenate([before[..., :coff], before[..., coff + c:]], -1))


def test_dw_bwd_tile_kernel_agrees(dev, tmp_path):
    names = list(dc.CASES)
    old = _child(tmp_path, {"LHN_DW_BWD_V1": "1"}, names, 1)
    for nm in names:
        new = dc.run(nm, dev)
        ref = dc.reference(nm)
        for k in ref:
            _close(old[f"{nm}/0/{k}"], ref[k], f"{nm} {k} (tile kernel)")
            _close(new[k], old[f"{nm}/0/{k}"].astype(np.float64), f"{nm} {k} new vs tile kernel")


def test_dw_bwd_deterministic_bits(tmp_path):
    names = ["bench_plain", "bench_bns", "bench_xgate_adds_nrep", "parity_32", "tail_20"]
    res = _child(tmp_path, {"LHN_DETERMINISTIC": "1"}, names, 2)
    for nm in names:
        ref = dc.reference(nm)
        for k in ref:
            np.testing.assert_array_equal(res[f"{nm}/0/{k}"], res[f"{nm}/1/{k}"], err_msg=f"{nm} {k}")
            _close(res[f"{nm}/0/{k}"], ref[k], f"{nm} {k} (deterministic)")
