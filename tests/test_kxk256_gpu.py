"""The dense 3x3 convolution with a side of 256 channels through the C ABI, per element against float64 (tests/kxk256_cases.py lists
the cases and which kernel instance each reaches): the K-sliced forward and data gradient (two 128-channel slices per tap inside
k_kxk<256, NT>), 256 features over gridDim.y, the weight gradient once per 128-channel input slice with Cout = 256 on 8 or 2 groups.
Bar as in tests/test_kxk_gpu.py: max(2e-5, 3 * e32) with e32 the error of torch's float32 CPU run of the same case, every `*_ok`
guard of the harness (slack behind dW replicas and the scratch, floats outside views, dz).  Every case but the refusals stops with
"unsupported channels" on a library without the 256-channel instances."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kxk256_cases as k2
import kxk_cases as kc
from conftest import parity_record

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FLOOR = 2e-5

_REF = {}


def _reference(kind, name):
    key = (kind, name)
    if key in _REF:
        return _REF[key]
    g = kc.inputs(kind, name)
    r64, r32 = kc.reference(kind, name, g), kc.reference(kind, name, g, torch.float32)
    e32 = {k: kc.rel_err(r32[k], r64[k]) for k in r64}
    if not name.startswith("big_"):      # (193 x 193 x 256: 38 MB per tensor, used by one test each)
        _REF[key] = (g, r64, e32)
    return g, r64, e32


def _check(kind, name, got, r64, e32, tag):
    """Every output of the reference, every element; every `*_ok` flag.  (All of these cases are on the plain path: dz holds dy.)"""
    bad = []
    for k, ref in r64.items():
        assert got[k].shape == ref.shape, f"{kind}:{name} {k}: shape {got[k].shape} vs {ref.shape}"
        err, bar = kc.rel_err(got[k], ref), max(FLOOR, 3 * e32[k])
        if not np.isfinite(err):
            err = float("inf")
        parity_record(f"kxk256/{tag}{kind}_{name}", **{f"{k}_err": err, f"{k}_e32": e32[k], f"{k}_bar": bar})
        print(f"kxk256 {tag}{kind}:{name} {k}: err {err:.3e} e32 {e32[k]:.3e} bar {bar:.3e}")
        if not err <= bar:
            bad.append(f"{k}: err {err:.3e} > bar {bar:.3e}")
    for k, v in got.items():
        if k.endswith("_ok") and not bool(v):
            bad.append(f"{k}: floats that must keep their bits changed")
    assert not bad, f"{tag}{kind}:{name}: " + "; ".join(bad)


def _child(tmp_path, env_extra, names, reps, timeout):
    out = str(tmp_path / "out.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("LHN_PLAIN", "LHN_DETERMINISTIC")}
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.join(HERE, "kxk256_cases.py"), out, str(reps)] + names, env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return dict(np.load(out))


def _of(res, full, rep):
    pre = f"{full}/{rep}/"
    return {k[len(pre):]: v for k, v in res.items() if k.startswith(pre)}


@pytest.mark.parametrize("name", list(k2.FWD))
def test_kxk256_fwd_matches_float64(dev, name):
    g, r64, e32 = _reference("fwd", name)
    _check("fwd", name, kc.run_fwd(name, dev, g), r64, e32, "")


@pytest.mark.parametrize("name", list(k2.BWD))
def test_kxk256_bwd_matches_float64(dev, name):
    assert kc.plain_path(k2.BWD[name])
    g, r64, e32 = _reference("bwd", name)
    _check("bwd", name, kc.run_bwd(name, dev, g), r64, e32, "")


def test_kxk256_bwd_stride2_lattice(dev):
    """One tap of W at a time (tests/test_kxk_gpu.py::test_kxk_bwd_stride2_lattice) with K = Cout sliced: tap (kh, kw) reaches only the
    input pixels of its parity class, every other pixel is stored as an exact zero, and the class meets the float64 bar."""
    name = "s2_256_256_odd_store"
    g, _, _ = _reference("bwd", name)
    for tap in range(9):
        kh, kw = divmod(tap, 3)
        g1 = dict(g)
        g1["w"] = torch.zeros_like(g["w"])
        g1["w"][:, :, kh, kw] = g["w"][:, :, kh, kw]
        r64, r32 = kc.reference_bwd(name, g1), kc.reference_bwd(name, g1, torch.float32)
        got = kc.run_bwd(name, dev, g1)
        _check("bwd", name, got, r64, {k: kc.rel_err(r32[k], r64[k]) for k in r64}, f"tap{tap}/")
        reached = np.zeros(got["dx"].shape[1:3], bool)
        reached[(kh + 1) % 2::2, (kw + 1) % 2::2] = True
        assert not got["dx"][:, ~reached].any(), f"{name} tap {tap}: a pixel outside the tap's parity class received a gradient"
        assert got["dx"][:, reached].any()


def test_kxk256_fwd_fused_finalize(dev):
    """fin != NULL with gridDim.y > 1: the last of gridDim.x * gridDim.y workgroups folds the statistics -- table, mean | invstd and
    running statistics against float64, the table outside the slice untouched, one ticket per workgroup."""
    g = k2.fin_inputs()
    r64, r32 = k2.reference_fwd_fin(g), k2.reference_fwd_fin(g, torch.float32)
    got = k2.run_fwd_fin(dev, g)
    assert bool(got["tickets_ok"]), got["tickets"]
    assert int(got["fin_nbt"][0]) == 6
    _check("fwd", "fin_256_256", {k: v for k, v in got.items() if k in r64 or k.endswith("_ok")}, r64,
           {k: kc.rel_err(r32[k], r64[k]) for k in r64}, "")


WT_CASES = [f"fwd:{n}" for n in k2.FWD if not n.startswith("big_")] + [f"bwd:{n}" for n in k2.BWD if n.startswith(("pair_", "s2_"))]


@pytest.mark.parametrize("full", WT_CASES)
def test_kxk256_wt_scratch_bits(dev, full):
    """wt_scratch = NULL (weights gathered from w[co][ci][tap], slice by slice) against the tap-major copy: the same products in the
    same order, so y and dx agree bit for bit."""
    kind, name = full.split(":")
    g, r64, e32 = _reference(kind, name)
    run = kc.run_fwd if kind == "fwd" else kc.run_bwd
    a, b = run(name, dev, g, wt=True), run(name, dev, g, wt=False)
    out = "y" if kind == "fwd" else "dx"
    np.testing.assert_array_equal(a[out], b[out], err_msg=full)
    _check(kind, name, b, r64, e32, "nowt/")
    assert bool(a["wt_ok"]) and "wt_ok" not in b


MT_CASES = [f"fwd:{n}" for n in k2.FWD if n.startswith("mt_")] + [f"bwd:{n}" for n in k2.BWD if n.startswith("mt_")]


def test_kxk256_deterministic_bits(dev, tmp_path):
    """LHN_DETERMINISTIC=1: grids sized for 2 CUs, so the 15-tile cases run NT = 4 (gridDim.y = 2 at 256 features) or NT = 2, several
    tiles per workgroup with the next tile's first slice in flight, and dW in 16 exclusive replicas; two runs agree bit for bit."""
    res = _child(tmp_path, {"LHN_DETERMINISTIC": "1"}, MT_CASES, 2, timeout=120)
    for full in MT_CASES:
        kind, name = full.split(":")
        _, r64, e32 = _reference(kind, name)
        a, b = _of(res, full, 0), _of(res, full, 1)
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{full} {k}")
        _check(kind, name, a, r64, e32, "deterministic/")


def test_kxk256_plain_switch_is_ignored(dev, tmp_path):
    """LHN_PLAIN=0 does not apply to a side of 256 channels (no dy-on-the-fly instance of the sliced kernels): dz holds dy after the
    call and the float64 bar holds."""
    names = ["bwd:pair_256_256", "bwd:pair_32_256", "bwd:pair_256_32"]
    res = _child(tmp_path, {"LHN_PLAIN": "0"}, names, 1, timeout=120)
    for full in names:
        kind, name = full.split(":")
        g, r64, e32 = _reference(kind, name)
        got = _of(res, full, 0)
        assert "dz" in got and "dz_unchanged_ok" not in got, f"{full}: the harness and the library disagree on the path"
        _check(kind, name, got, r64, e32, "LHN_PLAIN=0/")


@pytest.mark.parametrize("name", list(k2.FWD_REFUSE))
def test_kxk256_fwd_refuses(dev, name):
    rc, kept = kc.run_fwd(name, dev, expect_fail=True)
    assert rc != 0 and k2.FWD_REFUSE[name]["refuse"] in kc._lib.lib().lhn_last_error().decode()
    assert all(kept.values()), f"{name}: a refused call wrote to {[k for k, v in kept.items() if not v]}"


@pytest.mark.parametrize("name", list(k2.BWD_REFUSE))
def test_kxk256_bwd_refuses(dev, name):
    rc, kept = kc.run_bwd(name, dev, expect_fail=True)
    assert rc != 0 and k2.BWD_REFUSE[name]["refuse"] in kc._lib.lib().lhn_last_error().decode()
    assert all(kept.values()), f"{name}: a refused call wrote to {[k for k, v in kept.items() if not v]}"
