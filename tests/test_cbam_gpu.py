"""Direct C-ABI checks of the CBAM kernels (csrc/k_cbam.hip: lhn_cbam_fwd then lhn_cbam_bwd), per element against the float64
torch formulas of tests/cbam_cases.py: g, both channels of s, a, out, dp, dr, dW1, dW2, dW7 under the project's kernel bar
max(2e-5, 3 x the float32-on-the-CPU error of the same reference), relative to the largest magnitude of that output; the two
arg-max index tensors must EQUAL the float64 reference's.  Inputs are free of chaotic points (cbam_cases docstring).  Also: a
table with negative scales, views into sentinel-filled buffers, bitwise repeatability in the default mode, one child process
with LHN_DETERMINISTIC=1, and refusals that write nothing.

Scratch builds with one line of csrc/k_cbam.hip changed fail these cases (every case passes without the change):
  taps not mirrored in ds (sdq[th + kh][tw + kw])      dp, dW1, dW2 of the nine cases with more than one pixel (a 1 x 1 map sees
                                                       the centre tap only: n2c16_1x1 passes)
  the 1/C dropped from ds0                             dp, dW1, dW2 of all ten cases
  dmx routed to pixel 0 (amax == px -> 0 == px)        dp of the nine cases with more than one pixel"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cbam_cases as cc
from conftest import parity_record

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FLOOR = 2e-5        # the project's kernel-level floor (test_pw_gpu.FLOOR)

_REF = {}


def _reference(name):
    """(inputs, float64 reference, float32-on-the-CPU error per output); computed once per case and shared, never modified."""
    if name not in _REF:
        g = cc.inputs(name)
        r64, r32 = cc.reference(name, g), cc.reference(name, g, torch.float32)
        _REF[name] = (g, r64, {k: cc.rel_err(r32[k], r64[k]) for k in cc.OUTPUTS})
    return _REF[name]


def _check(name, got, tag=""):
    g, r64, e32 = _reference(name)
    bad = []
    for k in cc.INDEXES:
        same = np.array_equal(np.asarray(got[k]), r64[k])
        print(f"cbam {tag}{name} {k}: {'equal' if same else 'DIFFERENT'}")
        if not same:
            bad.append(f"{k}: {int((np.asarray(got[k]) != r64[k]).sum())} indices differ from the float64 reference")
    for k in cc.OUTPUTS:
        assert got[k].shape == r64[k].shape, (name, k, got[k].shape, r64[k].shape)
        err, bar = cc.rel_err(got[k], r64[k]), max(FLOOR, 3 * e32[k])
        err = err if np.isfinite(err) else float("inf")
        parity_record(f"cbam/{tag}{name}", **{f"{k}_err": err, f"{k}_e32": e32[k], f"{k}_bar": bar})
        print(f"cbam {tag}{name} {k}: err {err:.3e} e32 {e32[k]:.3e} bar {bar:.3e}")
        if not err <= bar:
            bad.append(f"{k}: err {err:.3e} > bar {bar:.3e}")
    for k, v in got.items():
        if k.endswith("_ok") and not bool(v):
            bad.append(f"{k}: floats outside the outputs changed")
    assert not bad, f"{tag}{name}: " + "; ".join(bad)


@pytest.mark.parametrize("name", cc.NAMES)
def test_cbam_matches_float64(dev, name):
    g, _, _ = _reference(name)
    rc_f, rc_b, got = cc.run(name, dev, g)
    assert rc_f == 0 and rc_b == 0, (rc_f, rc_b)
    _check(name, got)


@pytest.mark.parametrize("name", ["n3c32_9x33", "n2c128_14x14", "n1c16_33x40"])
def test_cbam_repeats_bits(dev, name):
    """No float atomics: the whole sequence run twice gives identical bits for every output, in the default mode."""
    g, _, _ = _reference(name)
    (_, _, a), (_, _, b) = cc.run(name, dev, g, reps=2)
    for k in cc.OUTPUTS + cc.INDEXES:
        assert np.array_equal(a[k], b[k]), k


def test_cbam_deterministic_mode(dev, tmp_path):
    """One child process with LHN_DETERMINISTIC=1: the same bar, and (no atomics anywhere) the same bits as the default mode."""
    names = ["n3c32_9x33", "n2c64_5x40", "n2c128_14x14"]
    out = str(tmp_path / "out.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "cbam_cases.py"), out] + names, env=dict(os.environ, LHN_DETERMINISTIC="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = np.load(out)
    for name in names:
        got = {k.split("/", 1)[1]: res[k] for k in res.files if k.startswith(name + "/")}
        _check(name, got, tag="det/")
        _, _, here = cc.run(name, dev, _reference(name)[0])
        for k in cc.OUTPUTS:
            assert np.array_equal(got[k], here[k]), (name, k)


@pytest.mark.parametrize("shape,why", [((2, 24, 5, 6), "multiple of 16"), ((1, 272, 3, 4), "<= 256")])
def test_cbam_refuses_channel_counts(dev, shape, why):
    rc_f, rc_b, res = cc.run(None, dev, cc.refusal_inputs(shape), shape=shape)
    assert rc_f != 0 and rc_b != 0 and res["untouched"], (rc_f, rc_b, res)
    assert why in res["error"], res["error"]


def test_cbam_refuses_null_scratch(dev):
    name = "n2c32_7x7"
    rc_f, rc_b, res = cc.run(name, dev, _reference(name)[0], null_scratch=True)
    assert rc_f == 0 and rc_b != 0 and res["bwd_untouched"], (rc_f, rc_b)
    from litehandnet_amd import _lib
    assert "null pointer" in _lib.lib().lhn_last_error().decode()
