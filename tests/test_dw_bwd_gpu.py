"""Direct C-ABI checks of the depthwise backward against a float64 torch reference, per element: the fused 3x3 kernels (dgrad +
wgrad with their fusions: dx accumulate, gradient addends, BatchNorm-backward sums of the producer, gated x / y, pooled-attention
gradient, parity sub-lattices, the direct dilation-2 path, channel tails, weight-gradient replicas) at the benchmark shape, at
128 x 128 and on small maps; the stride-2 kernel k_dws2_bwd_lds; the 7x7 tile kernel k_dwk_bwd_lds<7,1>; the row-gather pair
k_dw_bwd_data + k_dw_bwd_weight on the maps and kernel sizes that reach it.  The tile kernel the 3x3 replaced (LHN_DW_BWD_V1=1)
must agree, LHN_DW_GATHER=1 and LHN_XCD_ORDER=1 must meet the same bar, deterministic mode must repeat its bits, and calls
outside the supported set are refused without writing."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dw_bwd_cases as dc
from conftest import parity_record

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 2e-5          # relative to the largest magnitude of each output (float32 sums of <= 8k products vs float64)

_REF = {}


def _reference(name):
    """(inputs, float64 reference, float32-on-the-CPU error per output); computed once per case and shared."""
    if name not in _REF:
        g = dc.inputs(name)
        r64, r32 = dc.reference(name, g), dc.reference(name, g, torch.float32)
        _REF[name] = (g, r64, {k: dc.rel_err(r32[k], r64[k]) for k in r64})
    return _REF[name]


def _close(a, b, what):
    scale = max(float(np.abs(b).max()), 1e-30)
    err = float(np.abs(a.astype(np.float64) - b).max()) / scale
    assert err <= TOL, f"{what}: max rel err {err:.3e}"


def _check(name, got, r64, e32, tag):
    """Every output of the reference, every element, within max(TOL, 3 x the float32 error of the reference); every `*_ok` flag."""
    bad = []
    for k, ref in r64.items():
        assert got[k].shape == ref.shape, f"{name} {k}: shape {got[k].shape} vs {ref.shape}"
        err, bar = dc.rel_err(got[k], ref), max(TOL, 3 * e32[k])
        if not np.isfinite(err):
            err = float("inf")
        parity_record(f"dw/{tag}bwd_{name}", **{f"{k}_err": err, f"{k}_e32": e32[k], f"{k}_bar": bar})
        print(f"dw {tag}bwd:{name} {k}: err {err:.3e} e32 {e32[k]:.3e} bar {bar:.3e}")
        if not err <= bar:
            bad.append(f"{k}: err {err:.3e} > bar {bar:.3e}")
    for k, v in got.items():
        if k.endswith("_ok") and not bool(v):
            bad.append(f"{k}: floats outside the outputs changed")
    assert not bad, f"{tag}bwd:{name}: " + "; ".join(bad)


def _child(tmp_path, env_extra, names, reps, timeout=600):
    out = str(tmp_path / "out.npz")
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, os.path.join(HERE, "dw_bwd_cases.py"), out, str(reps)] + names, env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return dict(np.load(out))


def _of(res, name, rep):
    pre = f"{name}/{rep}/"
    return {k[len(pre):]: v for k, v in res.items() if k.startswith(pre)}


OLD_CASES = [n for n in dc.CASES if not n.startswith(dc.NEW_PREFIXES)]
NEW_CASES = [n for n in dc.CASES if n.startswith(dc.NEW_PREFIXES)]


@pytest.mark.parametrize("name", list(dc.CASES))
def test_dw_bwd_matches_float64(dev, name):
    g, ref, e32 = _reference(name)
    got = dc.run(name, dev, g)
    if name in OLD_CASES:
        for k in ref:
            _close(got[k], ref[k], f"{name} {k}")
    _check(name, got, ref, e32, "")
    _, _, _, cs, coff, c, _, _, k, stride, _ = dc.CASES[name]
    if cs > c:        # channels outside the view are untouched
        before = (g["prior"].numpy() if "prior" in g else np.full(g["x"].shape, 7.0, np.float32))
        np.testing.assert_array_equal(got["dx_outside"], np.concatenate([before[..., :coff], before[..., coff + c:]], -1))


def test_dw_bwd_tile_kernel_agrees(dev, tmp_path):
    names = OLD_CASES
    old = _child(tmp_path, {"LHN_DW_BWD_V1": "1"}, names, 1)
    for nm in names:
        g, ref, _ = _reference(nm)
        new = dc.run(nm, dev, g)
        for k in ref:
            _close(old[f"{nm}/0/{k}"], ref[k], f"{nm} {k} (tile kernel)")
            _close(new[k], old[f"{nm}/0/{k}"].astype(np.float64), f"{nm} {k} new vs tile kernel")


def test_dw_bwd_deterministic_bits(tmp_path):
    names = ["bench_plain", "bench_bns", "bench_xgate_adds_nrep", "parity_32", "tail_20"]
    res = _child(tmp_path, {"LHN_DETERMINISTIC": "1"}, names, 2)
    for nm in names:
        _, ref, _ = _reference(nm)
        for k in ref:
            np.testing.assert_array_equal(res[f"{nm}/0/{k}"], res[f"{nm}/1/{k}"], err_msg=f"{nm} {k}")
            _close(res[f"{nm}/0/{k}"], ref[k], f"{nm} {k} (deterministic)")


DET_NEW = [n for n in NEW_CASES if n.startswith(("s2_", "k7_"))] + ["g3_nrep", "g7_6x6"]


def test_dw_bwd_deterministic_bits_stride2_7x7(dev, tmp_path):
    """LHN_DETERMINISTIC=1 on the stride-2 and 7x7 kernels (and the gather pair): 2 CUs reported, so every grid loops over its
    tiles; 16 weight-gradient replicas, one writer each; two runs agree bit for bit."""
    res = _child(tmp_path, {"LHN_DETERMINISTIC": "1"}, DET_NEW, 2, timeout=240)
    for nm in DET_NEW:
        _, ref, e32 = _reference(nm)
        a, b = _of(res, nm, 0), _of(res, nm, 1)
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{nm} {k}")
        _check(nm, a, ref, e32, "deterministic/")


GATHER_CASES = [n for n in dc.CASES if not any(fl in dc.CASES[n][7].split() for fl in ("bns", "add0", "add1"))]


def test_dw_bwd_gather_switch(dev, tmp_path):
    """LHN_DW_GATHER=1: every case without fused BatchNorm sums or addends on k_dw_bwd_data + k_dw_bwd_weight -- the only way
    their stride-2, dilation-2 and 7x7 paths see maps of real size.  Same float64 bar."""
    assert all(dc.kernel_of(n, gather=True).startswith("k_dw_bwd_data<") for n in GATHER_CASES)
    res = _child(tmp_path, {"LHN_DW_GATHER": "1"}, GATHER_CASES, 1, timeout=240)
    for nm in GATHER_CASES:
        _, ref, e32 = _reference(nm)
        _check(nm, _of(res, nm, 0), ref, e32, "LHN_DW_GATHER/")


XCD_CASES = ["bench_plain", "tail_40_parity"]


def test_dw_bwd_xcd_order(dev, tmp_path):
    """LHN_XCD_ORDER=1 with the tile kernel (LHN_DW_BWD_V1=1): grids of 8 x 16 tiles that are a multiple of 8 * cgroups."""
    for nm in XCD_CASES:
        n, h, w, _, _, c, dil, _, _, _, _ = dc.CASES[nm]
        ps, cg = (2 if dil == 2 and w >= 16 else 1), (c + 31) // 32
        ntile = n * ps * ps * (((h + ps - 1) // ps + 7) // 8) * (((w + ps - 1) // ps + 15) // 16) * cg      # launch_dwk_bwd
        grid = min(256 * 4 - (256 * 4) % cg, ntile)                                                        # dw3_grid, 256 CUs
        assert grid % (8 * cg) == 0, f"{nm}: grid {grid} does not take the XCD order"                      # dw3_xchunk
    res = _child(tmp_path, {"LHN_XCD_ORDER": "1", "LHN_DW_BWD_V1": "1"}, XCD_CASES, 1, timeout=240)
    for nm in XCD_CASES:
        _, ref, e32 = _reference(nm)
        _check(nm, _of(res, nm, 0), ref, e32, "LHN_XCD_ORDER/")


@pytest.mark.parametrize("name", ["s2_16", "s2_34x66"])
def test_dw_bwd_stride2_reaches_every_pixel(dev, name):
    """Even maps: the last input row and column only meet tap 2 of the last output row / column; their gradient is not zero."""
    g, ref, _ = _reference(name)
    dx = dc.run(name, dev, g)["dx"]
    assert np.abs(ref["dx"][:, -1]).min() > 0 and np.abs(ref["dx"][:, :, -1]).min() > 0
    assert (dx[:, -1] != 0).all() and (dx[:, :, -1] != 0).all() and not (dx == 7.0).any()


@pytest.mark.parametrize("name", list(dc.REFUSE))
def test_dw_bwd_refuses(dev, name):
    rc, untouched = dc.run(name, dev, expect_fail=True)
    assert rc != 0 and dc.REFUSE[name][1] in dc._lib.lib().lhn_last_error().decode()      # refused for the reason the case names
    assert untouched, f"{name}: a refused call wrote to its outputs"
