"""Direct C-ABI checks of the dense 3x3 convolution, forward (lhn_conv_kxk_fwd) and backward (lhn_conv_kxk_bwd), per element
against a float64 torch reference: every instantiation of the implicit-GEMM kernel (forward, dgrad of the in-place dy, dgrad with
dy on the fly) and of the wgrad kernel (K-split, whole tiles per wave, cosplit with the exclusive flush, the atomic flush), the
stride-2 dgrad by pixel parity, the tap-major weight scratch in both layouts, k_dy_inplace with a gate and a pooled gradient,
channel-slice views, dx_accumulate, and persistent grids with more tiles than workgroups.  profiles/kxk_instances.md lists which case
reaches which instantiation.  LHN_PLAIN=0 and LHN_PLAIN=1 must meet the same bar, deterministic mode must repeat its bits, and
calls outside the supported set are refused without writing -- dz included."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kxk_cases as kc
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
    g = kc.inputs(kind, name)
    r64, r32 = kc.reference(kind, name, g), kc.reference(kind, name, g, torch.float32)
    e32 = {k: kc.rel_err(r32[k], r64[k]) for k in r64}
    if not name.startswith("big_"):      # (the 257 x 257 cases: up to 34 MB per tensor, used by one test each)
        _REF[key] = (g, r64, e32)
    return g, r64, e32


def _check(kind, name, got, r64, e32, tag, plain=None):
    """Every output of the reference, every element; every `*_ok` flag (floats that must keep their bits).  `dz` after a backward
    call is dy where the plain path ran (`plain`: what the dispatch rule says for this case and environment) and the input bits
    where it did not."""
    bad = []
    for k, ref in r64.items():
        if kind == "bwd" and k == "dz" and not plain:
            if "dz" in got or not bool(got.get("dz_unchanged_ok", False)):
                bad.append("dz: dy on the fly must leave dz as it was")
            continue
        assert got[k].shape == ref.shape, f"{kind}:{name} {k}: shape {got[k].shape} vs {ref.shape}"
        err, bar = kc.rel_err(got[k], ref), max(FLOOR, 3 * e32[k])
        if not np.isfinite(err):
            err = float("inf")
        parity_record(f"kxk/{tag}{kind}_{name}", **{f"{k}_err": err, f"{k}_e32": e32[k], f"{k}_bar": bar})
        print(f"kxk {tag}{kind}:{name} {k}: err {err:.3e} e32 {e32[k]:.3e} bar {bar:.3e}")
        if not err <= bar:
            bad.append(f"{k}: err {err:.3e} > bar {bar:.3e}")
    for k, v in got.items():
        if k.endswith("_ok") and not bool(v):
            bad.append(f"{k}: floats outside the outputs changed")
    assert not bad, f"{tag}{kind}:{name}: " + "; ".join(bad)


def _default_plain(c):
    return "dpool" in c["flags"] or c["cin"] * c["cout"] >= 64 * 64


def _child(tmp_path, env_extra, names, reps, timeout):
    out = str(tmp_path / "out.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("LHN_PLAIN", "LHN_DETERMINISTIC")}
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.join(HERE, "kxk_cases.py"), out, str(reps)] + names, env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return dict(np.load(out))


def _of(res, full, rep):
    pre = f"{full}/{rep}/"
    return {k[len(pre):]: v for k, v in res.items() if k.startswith(pre)}


@pytest.mark.parametrize("name", list(kc.FWD))
def test_kxk_fwd_matches_float64(dev, name):
    g, r64, e32 = _reference("fwd", name)
    _check("fwd", name, kc.run_fwd(name, dev, g), r64, e32, "")


@pytest.mark.parametrize("name", list(kc.BWD))
def test_kxk_bwd_matches_float64(dev, name):
    g, r64, e32 = _reference("bwd", name)
    _check("bwd", name, kc.run_bwd(name, dev, g), r64, e32, "", plain=kc.plain_path(kc.BWD[name]))


@pytest.mark.parametrize("name", ["s2_32_32_odd_store", "s2_128_64_even_store"])
def test_kxk_bwd_stride2_lattice(dev, name):
    """One tap of W at a time: with stride 2, tap (kh, kw) reaches only the input pixels with ih = kh + 1, iw = kw + 1 (mod 2) --
    the parity class whose tap list holds it.  Every other pixel is stored as an exact zero, and the class meets the float64 bar."""
    g, _, _ = _reference("bwd", name)
    for tap in range(9):
        kh, kw = divmod(tap, 3)
        g1 = dict(g)
        g1["w"] = torch.zeros_like(g["w"])
        g1["w"][:, :, kh, kw] = g["w"][:, :, kh, kw]
        r64, r32 = kc.reference_bwd(name, g1), kc.reference_bwd(name, g1, torch.float32)
        got = kc.run_bwd(name, dev, g1)
        _check("bwd", name, got, r64, {k: kc.rel_err(r32[k], r64[k]) for k in r64}, f"tap{tap}/", plain=kc.plain_path(kc.BWD[name]))
        reached = np.zeros(got["dx"].shape[1:3], bool)
        reached[(kh + 1) % 2::2, (kw + 1) % 2::2] = True
        assert not got["dx"][:, ~reached].any(), f"{name} tap {tap}: a pixel outside the tap's parity class received a gradient"
        assert got["dx"][:, reached].any()


WT_CASES = [f"fwd:{n}" for n in kc.FWD if n.startswith(("pair_", "tiny_", "view_", "s2_", "nostats_", "tail_"))] + \
           [f"bwd:{n}" for n in kc.BWD if n.startswith(("pair_", "s2_"))]


@pytest.mark.parametrize("full", WT_CASES)
def test_kxk_wt_scratch_bits(dev, full):
    """wt_scratch = NULL (weights gathered from w[co][ci][tap]) against the tap-major copy: the same products in the same order, so
    y and dx agree bit for bit (the statistics and dW go through atomics and are held to the float64 bar instead)."""
    kind, name = full.split(":")
    g, r64, e32 = _reference(kind, name)
    if kind == "fwd":
        a, b = kc.run_fwd(name, dev, g, wt=True), kc.run_fwd(name, dev, g, wt=False)
        np.testing.assert_array_equal(a["y"], b["y"], err_msg=full)
        _check(kind, name, b, r64, e32, "nowt/")
    else:
        a, b = kc.run_bwd(name, dev, g, wt=True), kc.run_bwd(name, dev, g, wt=False)
        np.testing.assert_array_equal(a["dx"], b["dx"], err_msg=full)
        _check(kind, name, b, r64, e32, "nowt/", plain=kc.plain_path(kc.BWD[name]))
    assert bool(a["wt_ok"]) and "wt_ok" not in b


@pytest.mark.parametrize("name", ["pair_64_64", "pair_32_128", "s2_128_64_odd", "tail_64_40", "mt_128_128"])
def test_kxk_fwd_repeats_bits(dev, name):
    """stats = NULL and fin = NULL leave the forward without atomics: two calls give the same bits."""
    g, _, _ = _reference("fwd", name)
    a, b = kc.run_fwd(name, dev, g, stats=False), kc.run_fwd(name, dev, g, stats=False)
    assert "stats_sum" not in a
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{name} {k}")


MT_CASES = [f"fwd:{n}" for n in kc.FWD if n.startswith("mt_")] + [f"bwd:{n}" for n in kc.BWD if n.startswith("mt_")]


@pytest.mark.parametrize("plain", [None, "0", "1"])
def test_kxk_deterministic_bits(dev, tmp_path, plain):
    """LHN_DETERMINISTIC=1: the library sizes its grids for 2 CUs, so the 15-tile cases run NT = all feature tiles of a block, loop
    over several tiles per workgroup with the next tile's loads in flight, and flush dW into 16 exclusive replicas; two runs agree
    bit for bit.  With LHN_PLAIN=0 / 1 on top, every NT > 1 dgrad instance runs in both of its dy forms."""
    env = {"LHN_DETERMINISTIC": "1"}
    if plain is not None:
        env["LHN_PLAIN"] = plain
    names = MT_CASES if plain is None else [n for n in MT_CASES if n.startswith("bwd:")]
    res = _child(tmp_path, env, names, 2, timeout=120)
    for full in names:
        kind, name = full.split(":")
        _, r64, e32 = _reference(kind, name)
        a, b = _of(res, full, 0), _of(res, full, 1)
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{full} {k}")
        is_plain = kind == "bwd" and (_default_plain(kc.BWD[name]) if plain is None else plain == "1")
        _check(kind, name, a, r64, e32, "deterministic/" + (f"LHN_PLAIN={plain}/" if plain is not None else ""), plain=is_plain)


PLAIN_CASES = [f"bwd:{n}" for n in kc.BWD if n.startswith(("pair_", "rep1_"))]       # (none of them has a pooled gradient)
DPOOL_CASES = ["bwd:full_64_64", "bwd:full_32_128", "bwd:dpool_32_32"]


@pytest.mark.parametrize("value", ["0", "1"])
def test_kxk_plain_switch_paths_agree(dev, tmp_path, value):
    """LHN_PLAIN=0: dy on the fly in the dgrad and the wgrad for every channel pair, dz only read;  LHN_PLAIN=1: dz := dy first for
    every pair.  Same float64 bar as the default choice.  A pooled gradient exists only in k_dy_inplace, so those cases stay on the
    plain path whatever the switch says."""
    res = _child(tmp_path, {"LHN_PLAIN": value}, PLAIN_CASES + DPOOL_CASES, 1, timeout=120)
    for full in PLAIN_CASES + DPOOL_CASES:
        kind, name = full.split(":")
        _, r64, e32 = _reference(kind, name)
        got = _of(res, full, 0)
        is_plain = value == "1" or full in DPOOL_CASES
        assert ("dz" in got) == is_plain, f"{full}: the test and the library disagree on the path"
        _check(kind, name, got, r64, e32, f"LHN_PLAIN={value}/", plain=is_plain)


@pytest.mark.parametrize("name", list(kc.FWD_REFUSE))
def test_kxk_fwd_refuses(dev, name):
    rc, kept = kc.run_fwd(name, dev, expect_fail=True)
    assert rc != 0 and kc.FWD_REFUSE[name]["refuse"] in kc._lib.lib().lhn_last_error().decode()      # refused for the reason the case names
    assert all(kept.values()), f"{name}: a refused call wrote to {[k for k, v in kept.items() if not v]}"


@pytest.mark.parametrize("name", list(kc.BWD_REFUSE))
def test_kxk_bwd_refuses(dev, name):
    rc, kept = kc.run_bwd(name, dev, expect_fail=True)
    assert rc != 0 and kc.BWD_REFUSE[name]["refuse"] in kc._lib.lib().lhn_last_error().decode()      # refused for the reason the case names
    assert all(kept.values()), f"{name}: a refused call wrote to {[k for k, v in kept.items() if not v]}"
