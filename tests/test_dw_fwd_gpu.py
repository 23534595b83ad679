"""Direct C-ABI checks of the depthwise forward (lhn_conv_dw_fwd / _fwd2 / _fwd3), per element against a float64 torch reference:
every instantiation of the tiled kernel k_dwk_fwd_lds (3x3, 3x3 on parity sub-lattices, direct dilation 2, 7x7, two summed
sources with sum_out), the stride-2 kernel k_dws2_fwd_lds, the row-gather kernel k_dw_fwd<1|3|5|7> with each of its statistics
reductions, and the fused BatchNorm finalize.  LHN_DW_GATHER=1 and LHN_XCD_ORDER=1 must meet the same bar, deterministic mode
must repeat its bits, a forward without statistics must repeat its bits, and calls outside the supported set are refused
without writing.  profiles/dw_instances.md lists which case reaches which kernel."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dw_fwd_cases as fc
from conftest import parity_record

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FLOOR = 2e-5        # the project's kernel-level floor (test_pw_gpu.FLOOR)

_REF = {}


def _reference(name):
    """(inputs, float64 reference, float32-on-the-CPU error per output); computed once per case and shared."""
    if name not in _REF:
        g = fc.inputs(name)
        r64, r32 = fc.reference(name, g), fc.reference(name, g, torch.float32)
        _REF[name] = (g, r64, {k: fc.rel_err(r32[k], r64[k]) for k in r64})
    return _REF[name]


def _check(name, got, r64, e32, tag, skip=()):
    """Every output of the reference, every element; every `*_ok` flag (floats that must keep their bits)."""
    bad = []
    for k, ref in r64.items():
        if k in skip:
            continue
        assert got[k].shape == ref.shape, f"{name} {k}: shape {got[k].shape} vs {ref.shape}"
        err, bar = fc.rel_err(got[k], ref), max(FLOOR, 3 * e32[k])
        if not np.isfinite(err):
            err = float("inf")
        parity_record(f"dw/{tag}fwd_{name}", **{f"{k}_err": err, f"{k}_e32": e32[k], f"{k}_bar": bar})
        print(f"dw {tag}fwd:{name} {k}: err {err:.3e} e32 {e32[k]:.3e} bar {bar:.3e}")
        if not err <= bar:
            bad.append(f"{k}: err {err:.3e} > bar {bar:.3e}")
    for k, v in got.items():
        if k.endswith("_ok") and not bool(v):
            bad.append(f"{k}: floats outside the outputs changed")
    assert not bad, f"{tag}fwd:{name}: " + "; ".join(bad)


def _child(tmp_path, env_extra, names, reps, timeout=240):
    out = str(tmp_path / "out.npz")
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, os.path.join(HERE, "dw_fwd_cases.py"), out, str(reps)] + names, env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return dict(np.load(out))


def _of(res, name, rep):
    pre = f"{name}/{rep}/"
    return {k[len(pre):]: v for k, v in res.items() if k.startswith(pre)}


@pytest.mark.parametrize("name", list(fc.CASES))
def test_dw_fwd_matches_float64(dev, name):
    g, r64, e32 = _reference(name)
    got = fc.run(name, dev, g)
    _check(name, got, r64, e32, "")
    if "fin" in fc.CASES[name]["flags"]:
        assert int(got["fin_nbt"][0]) == 6                       # 5 before the call
        parity_record(f"dw/fwd_{name}", fused_equals_separate_finalize_bits=bool(got["sep_bits_equal"]))
        print(f"dw fwd:{name} fused finalize == separate lhn_bn_finalize, bit for bit: {bool(got['sep_bits_equal'])}")
        for k in ("scale", "shift", "rmean", "rvar"):            # the separate launch meets the same bar
            err, bar = fc.rel_err(got[f"sep_{k}"], r64[f"fin_{k}"]), max(FLOOR, 3 * e32[f"fin_{k}"])
            assert err <= bar, f"{name} lhn_bn_finalize {k}: err {err:.3e} > bar {bar:.3e}"


GATHER_CASES = [n for n in fc.CASES if n.startswith(("lds3_", "par_", "d2_", "k7_", "s2_"))]       # groups 1-4 and 6


def test_dw_fwd_gather_switch(dev, tmp_path):
    """LHN_DW_GATHER=1: the tiled and the stride-2 shapes on k_dw_fwd<3|7> -- the only way its stride-2 and dilation-2 paths see
    maps of real size.  Same float64 bar."""
    assert all(fc.kernel_of(n, gather=True).startswith("k_dw_fwd<") for n in GATHER_CASES)
    res = _child(tmp_path, {"LHN_DW_GATHER": "1"}, GATHER_CASES, 1)
    for name in GATHER_CASES:
        _, r64, e32 = _reference(name)
        _check(name, _of(res, name, 0), r64, e32, "LHN_DW_GATHER/")


XCD_CASES = ["lds3_notab", "par_32"]


def test_dw_fwd_xcd_order(dev, tmp_path):
    """LHN_XCD_ORDER=1: the launch grid of these cases is a multiple of 8 * cgroups, so the tiles are dealt in XCD order."""
    for name in XCD_CASES:
        grid, xchunk = fc.xcd_grid(name)
        assert xchunk > 0 and grid % 8 == 0, f"{name}: grid {grid} does not take the XCD order"
    res = _child(tmp_path, {"LHN_XCD_ORDER": "1"}, XCD_CASES, 1)
    for name in XCD_CASES:
        _, r64, e32 = _reference(name)
        _check(name, _of(res, name, 0), r64, e32, "LHN_XCD_ORDER/")


DET_CASES = ["lds3_16", "lds3_c40", "par_17x19", "d2_12x13_c20", "k7_16", "ex_9x37_c20_so", "s2_34x66", "g3_4x4", "g3_c40", "g1_w", "g5_9",
             "g7_6x6"]


def test_dw_fwd_deterministic_bits(dev, tmp_path):
    """LHN_DETERMINISTIC=1: the library reports 2 CUs, so every persistent grid loops over many tiles (the tile loop and the
    one-tile-ahead prefetch at small shapes); two runs agree bit for bit, statistics included."""
    res = _child(tmp_path, {"LHN_DETERMINISTIC": "1"}, DET_CASES, 2)
    for name in DET_CASES:
        _, r64, e32 = _reference(name)
        a, b = _of(res, name, 0), _of(res, name, 1)
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{name} {k}")
        _check(name, a, r64, e32, "deterministic/")


@pytest.mark.parametrize("name", fc.NOSTATS_TWICE)
def test_dw_fwd_repeats_bits(dev, name):
    """Without statistics the forward has no atomics: two calls give the same bits (and meet the bar)."""
    g, r64, e32 = _reference(name)
    a, b = fc.run(name, dev, g, stats=False), fc.run(name, dev, g, stats=False)
    assert "stats_sum" not in a
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{name} {k}")
    _check(name, a, r64, e32, "nostats/", skip=("stats_sum", "stats_sq"))


@pytest.mark.parametrize("name", list(fc.REFUSE))
def test_dw_fwd_refuses(dev, name):
    rc, untouched = fc.run(name, dev, expect_fail=True)
    assert rc != 0 and fc.REFUSE[name]["refuse"] in fc._lib.lib().lhn_last_error().decode()      # refused for the reason the case names
    assert untouched, f"{name}: a refused call wrote to its outputs"
