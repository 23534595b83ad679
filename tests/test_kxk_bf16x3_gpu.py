"""Direct C-ABI checks of the split-bf16 dense 3x3 convolution (lhn_conv_kxk_fwd_bf16x3), per element, against two float64
references (tests/kxk_bf16x3_cases.py):
    S, the three-term split sum the kernel is meant to compute -- bar: the project's kernel rule, max(2e-5, 3 x the error of the same
       three convolutions evaluated in float32 on the CPU) of max |S|.  A dropped or doubled cross term misses it by about 80 x.
    T, the true convolution -- bar per element: 3.1 * 2^-16 * conv64(|v|, |w|) plus the bar above.
An integer case must come back bit for bit; the split-weight scratch must hold torch's bfloat16 conversion, ties included; repeated
calls, relay = 0 and LHN_DETERMINISTIC=1 must give the same bits; calls outside the supported set are refused without writing."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kxk_bf16x3_cases as bc
from conftest import parity_record

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

_REF = {}


def _reference(name):
    """(inputs, references) of a case, computed once and shared."""
    if name not in _REF:
        g = bc.inputs(name)
        _REF[name] = (g, bc.reference(name, g))
    return _REF[name]


def _check(name, got, r, tag=""):
    y = got["y"].astype(np.float64)
    assert y.shape == r["S"].shape, (name, y.shape, r["S"].shape)
    peak = max(float(np.abs(r["S"]).max()), 1e-30)
    e32, bar = bc.bars(r)
    err_s = float(np.abs(y - r["S"]).max()) / peak
    slack_t = bc.BOUND * r["A"] + bar * peak
    ratio_t = float((np.abs(y - r["T"]) / np.maximum(slack_t, 1e-300)).max())
    err_t = float(np.abs(y - r["T"]).max()) / max(float(np.abs(r["T"]).max()), 1e-30)
    print(f"kxk_bf16x3 {tag}{name}: vs S err {err_s:.3e} e32 {e32:.3e} bar {bar:.3e}; vs T err {err_t:.3e}, worst share of the per-element bar {ratio_t:.3f}")
    parity_record(f"kxk_bf16x3/{tag}{name}", S_err=err_s, S_e32=e32, S_bar=bar, T_err=err_t, T_share_of_bar=ratio_t)
    bad = []
    if not err_s <= bar:
        bad.append(f"against the split sum: err {err_s:.3e} > bar {bar:.3e}")
    if not ratio_t <= 1.0:
        bad.append(f"against the true convolution: {ratio_t:.3f} of the per-element bar")
    bad += [f"{k} failed" for k, v in got.items() if k.endswith("_ok") and not bool(v)]
    assert not bad, f"{tag}{name}: " + "; ".join(bad)


@pytest.mark.parametrize("name", [n for n in bc.CASES if "ints" not in bc.CASES[n]["flags"]])
def test_matches_split_sum_and_true_convolution(dev, name):
    g, r = _reference(name)
    _check(name, bc.run(name, dev, g), r)


@pytest.mark.parametrize("name", [n for n in bc.CASES if "ints" in bc.CASES[n]["flags"]])
def test_integer_case_is_exact(dev, name):
    """v and w are integers in [-4, 4]: both lo parts are zero and every partial sum is an integer below 2^24, so the output equals the
    float64 convolution bit for bit -- indexing, tap orientation and padding, independent of any tolerance."""
    g, r = _reference(name)
    got = bc.run(name, dev, g)
    np.testing.assert_array_equal(got["y"].astype(np.float64), r["T"], err_msg=name)
    assert bool(got["y_outside_ok"]) and bool(got["y_written_ok"]) and bool(got["scratch_ok"])


def test_single_tap_weights_find_their_pixel(dev):
    """One tap of W at a time on the integer case: tap (kh, kw) must read pixel (h + kh - 1, w + kw - 1) and zeros outside the map."""
    name = "ints_32_64"
    g, _ = _reference(name)
    for tap in range(9):
        kh, kw = divmod(tap, 3)
        g1 = dict(g)
        g1["w"] = torch.zeros_like(g["w"])
        g1["w"][:, :, kh, kw] = g["w"][:, :, kh, kw]
        np.testing.assert_array_equal(bc.run(name, dev, g1)["y"].astype(np.float64), bc.reference(name, g1)["T"], err_msg=f"tap {tap}")


def test_split_image_agrees_with_torch_on_ties(dev):
    """Weights that sit exactly half-way between two bfloat16 values (both parities of the kept mantissa), their neighbours one float32
    ulp away, zeros, a subnormal and the largest finite bfloat16: the scratch equals torch's .to(torch.bfloat16) of w and of w - hi."""
    name = "pair_32_32"
    g = dict(_reference(name)[0])
    bits = []
    for base in (0x3F800000, 0x3F810000, 0xBF820000, 0x40FF0000, 0x00800000, 0x7F000000):
        bits += [base + 0x8000, base + 0x7FFF, base + 0x8001, base + 0x18000, base]
    bits += [0x00000000, 0x80000000, 0x00000001, 0x7F7F0000, 0x3F7FFFFF]
    w = g["w"].clone().view(-1)
    w[:len(bits)] = torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.float32).copy())
    g["w"] = w.view_as(g["w"]).contiguous()
    got = bc.run(name, dev, g)
    assert bool(got["scratch_ok"])


@pytest.mark.parametrize("name", ["pair_64_64", "pair_128_128", "view_128_32", "tiny_32_128", "ints_128_128"])
def test_repeats_bits_with_and_without_relay(dev, name):
    g, _ = _reference(name)
    a = bc.run(name, dev, g)
    b = bc.run(name, dev, g)
    c = bc.run(name, dev, g, relay=0, scratch=a["scratch"])
    for other in (b, c):
        np.testing.assert_array_equal(a["y"].view(np.int32), other["y"].view(np.int32), err_msg=name)
        assert bool(other["scratch_ok"]) and bool(other["y_outside_ok"]) and bool(other["y_written_ok"])


def test_deterministic_mode_gives_the_default_bits(dev, tmp_path):
    """A child process under LHN_DETERMINISTIC=1 (twice each) against this process's default mode: the kernel has no atomics and no
    grid-dependent order, so all three agree bit for bit."""
    names = [f"pair_{ci}_{co}" for ci, co in bc.PAIRS] + ["view_64_64", "above_128_64"]
    out = str(tmp_path / "out.npz")
    env = dict(os.environ, LHN_DETERMINISTIC="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "kxk_bf16x3_cases.py"), out, "2"] + names, env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = dict(np.load(out))
    for name in names:
        g, ref = _reference(name)
        here = bc.run(name, dev, g)
        for rep in (0, 1):
            np.testing.assert_array_equal(res[f"{name}/{rep}/y"].view(np.int32), here["y"].view(np.int32), err_msg=f"{name} run {rep}")
            assert all(bool(res[f"{name}/{rep}/{k}"]) for k in ("y_outside_ok", "y_written_ok", "scratch_ok"))
        _check(name, {"y": res[f"{name}/0/y"]}, ref, "deterministic/")


@pytest.mark.parametrize("name", list(bc.REFUSE))
def test_refuses_without_writing(dev, name):
    rc, kept = bc.run(name, dev, expect_fail=True)
    assert rc == 1 and bc.REFUSE[name]["refuse"] in bc._lib.lib().lhn_last_error().decode()      # invalid argument, for the reason the case names
    assert all(kept.values()), f"{name}: a refused call wrote to {[k for k, v in kept.items() if not v]}"
