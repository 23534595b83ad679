"""Direct C-ABI checks of the 1x1 convolution, forward (lhn_conv_pw_fwd2) and backward (lhn_conv_pw_bwd3), per element against a
float64 torch reference: every instantiation of the register-resident-W and LDS-W forward kernels, K / output slicing, the
one-pass K = 256 forward, the padded 21-in-24 head with its NCHW store, summed-on-load sources with sum_out, the fused backward
in every (tile, NTO) shape with its NCHW and BatchNorm-sum flavours, the split backward (k_dy_inplace, dgrad, wgrad) in every
slice pattern, and persistent grids with more tiles than workgroups.  The A/B switches LHN_PW_LDSW=1 and LHN_PW_K256=0 must meet
the same bar, deterministic mode must repeat its bits, and calls outside the supported set are refused without writing."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pw_cases as pc
from conftest import parity_record

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FLOOR = 2e-5        # the project's kernel-level floor (test_dw_bwd_gpu.TOL): float32 sums against float64, relative to the largest magnitude

_REF = {}


def _reference(kind, name):
    """(inputs, float64 reference, float32-on-the-CPU error per output); computed once per case and shared."""
    key = (kind, name)
    if key in _REF:
        return _REF[key]
    g = pc.inputs(kind, name)
    r64, r32 = pc.reference(kind, name, g), pc.reference(kind, name, g, torch.float32)
    e32 = {k: pc.rel_err(r32[k], r64[k]) for k in r64}
    if not name.startswith("big_"):      # (the 257 x 257 cases: 68 MB per tensor, used by one test each)
        _REF[key] = (g, r64, e32)
    return g, r64, e32


def _check(kind, name, got, r64, e32, tag):
    """Every output of the reference, every element; every `*_ok` flag (floats that must keep their bits)."""
    bad = []
    for k, ref in r64.items():
        assert got[k].shape == ref.shape, f"{kind}:{name} {k}: shape {got[k].shape} vs {ref.shape}"
        err, bar = pc.rel_err(got[k], ref), max(FLOOR, 3 * e32[k])
        if not np.isfinite(err):
            err = float("inf")
        parity_record(f"pw/{tag}{kind}_{name}", **{f"{k}_err": err, f"{k}_e32": e32[k], f"{k}_bar": bar})
        print(f"pw {tag}{kind}:{name} {k}: err {err:.3e} e32 {e32[k]:.3e} bar {bar:.3e}")
        if not err <= bar:
            bad.append(f"{k}: err {err:.3e} > bar {bar:.3e}")
    for k, v in got.items():
        if k.endswith("_ok") and not bool(v):
            bad.append(f"{k}: floats outside the outputs changed")
    assert not bad, f"{tag}{kind}:{name}: " + "; ".join(bad)


def _child(tmp_path, env_extra, names, reps, timeout):
    out = str(tmp_path / "out.npz")
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, os.path.join(HERE, "pw_cases.py"), out, str(reps)] + names, env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return dict(np.load(out))


def _of(res, full, rep):
    pre = f"{full}/{rep}/"
    return {k[len(pre):]: v for k, v in res.items() if k.startswith(pre)}


@pytest.mark.parametrize("name", list(pc.FWD))
def test_pw_fwd_matches_float64(dev, name):
    g, r64, e32 = _reference("fwd", name)
    got = pc.run_fwd(name, dev, g)
    _check("fwd", name, got, r64, e32, "")
    c = pc.FWD[name]
    if "w_rows" in c:       # rows beyond the weight tensor: zero weights and zero bias, so the store writes exact zeros
        assert not got["y_nchw"][:, c["w_rows"]:].any()
    if "w_cols" in c:       # NaN in the pad channels of x must not reach y
        assert np.isfinite(got["y"]).all()


@pytest.mark.parametrize("name", list(pc.BWD))
def test_pw_bwd_matches_float64(dev, name):
    g, r64, e32 = _reference("bwd", name)
    got = pc.run_bwd(name, dev, g)
    _check("bwd", name, got, r64, e32, "")
    if pc.BWD[name]["stride"] == 2:       # pixels off the stride lattice receive nothing
        dx = got["dx"]
        lattice = np.zeros(dx.shape[1:3], bool)
        lattice[::2, ::2] = True
        assert not dx[:, ~lattice].any()


SWITCH_CASES = [f"fwd:{n}" for n in pc.FWD if n.startswith(("wr_", "k256_"))] + [f"bwd:{n}" for n in pc.BWD if n.startswith("split_")]


@pytest.mark.parametrize("switch", ["LHN_PW_LDSW=1", "LHN_PW_K256=0"])
def test_pw_switch_paths_agree(dev, tmp_path, switch):
    """LHN_PW_LDSW=1: no register-W kernel (forward on k_pw_fwd, the split backward's dgrad on the one-tap implicit GEMM);
    LHN_PW_K256=0: K = 256 as two slices, the second accumulating.  Same float64 bar as the default paths."""
    k, v = switch.split("=")
    res = _child(tmp_path, {k: v}, SWITCH_CASES, 1, timeout=240)
    for full in SWITCH_CASES:
        kind, name = full.split(":")
        _, r64, e32 = _reference(kind, name)
        _check(kind, name, _of(res, full, 0), r64, e32, f"{k}/")


DET_CASES = ["fwd:wr_64_64", "fwd:tail_40_80", "fwd:slice_160_96", "fwd:k256_256_256", "fwd:big_32_32", "bwd:fused_64_64", "bwd:bns_64_64_16",
             "bwd:split_256_128", "bwd:head_64_24"]


def test_pw_deterministic_bits(dev, tmp_path):
    """LHN_DETERMINISTIC=1: grids of at most 16 workgroups, so every instantiation loops over many tiles; two runs agree bit for bit."""
    res = _child(tmp_path, {"LHN_DETERMINISTIC": "1"}, DET_CASES, 2, timeout=240)
    for full in DET_CASES:
        kind, name = full.split(":")
        _, r64, e32 = _reference(kind, name)
        a, b = _of(res, full, 0), _of(res, full, 1)
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{full} {k}")
        _check(kind, name, a, r64, e32, "deterministic/")


@pytest.mark.parametrize("name", ["wr_64_64", "tail_40_80", "k256_256_256", "ms_64_64_e2"])
def test_pw_fwd_repeats_bits(dev, name):
    """Without statistics the forward has no atomics: two calls give the same bits."""
    g, _, _ = _reference("fwd", name)
    a, b = pc.run_fwd(name, dev, g, stats=False), pc.run_fwd(name, dev, g, stats=False)
    assert "stats_sum" not in a
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{name} {k}")


@pytest.mark.parametrize("name", list(pc.FWD_REFUSE))
def test_pw_fwd_refuses(dev, name):
    rc, untouched = pc.run_fwd(name, dev, expect_fail=True)
    assert rc != 0 and pc.FWD_REFUSE[name]["refuse"] in pc._lib.lib().lhn_last_error().decode()      # refused for the reason the case names
    assert untouched, f"{name}: a refused call wrote to its outputs"


@pytest.mark.parametrize("name", list(pc.BWD_REFUSE))
def test_pw_bwd_refuses(dev, name):
    rc, untouched = pc.run_bwd(name, dev, expect_fail=True)
    assert rc != 0 and pc.BWD_REFUSE[name]["refuse"] in pc._lib.lib().lhn_last_error().decode()      # refused for the reason the case names
    assert untouched, f"{name}: a refused call wrote to its outputs"
