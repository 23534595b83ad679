"""Direct C-ABI checks of the stem convolution (lhn_conv_stem_fwd / lhn_conv_stem_bwd), per element against a float64 torch
reference: the MFMA pairs for 3x3 -> 32 and 7x7 -> 64 and the direct pair k_stem_fwd / k_stem_bwd<K,KR>, at pixel counts that are no
multiple of the tile (dead pixels, waves without a pixel, tiles that straddle two images), odd image sizes, maps smaller than the
kernel, stride 1, no padding, with the fused BatchNorm finalize and every gradient-side input.  LHN_DW_GATHER=1 (the MFMA shapes on
the direct kernels) must meet the same bar, deterministic mode (2 CUs: the tile loop and the prefetch) must repeat its bits, a
forward without statistics must repeat its bits, a large mean must not cost the MFMA forwards the batch variance, and calls
outside the supported set are refused without writing.  tests/stem_cases.py lists which case reaches which kernel."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import stem_cases as sc
from conftest import parity_record

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FLOOR = 2e-5        # the project's kernel-level floor (test_pw_gpu.FLOOR)

_IN, _REF, _CHILD = {}, {}, {}


def _reference(name, kind):
    """(inputs, float64 reference, float32-on-the-CPU error per output); computed once per case and shared."""
    if (name, kind) not in _REF:
        g = _IN[name] = _IN.get(name) or sc.inputs(name)
        r64, r32 = sc.reference(name, g, kind=kind), sc.reference(name, g, torch.float32, kind=kind)
        _REF[(name, kind)] = (g, r64, {k: sc.rel_err(r32[k], r64[k]) for k in r64})
    return _REF[(name, kind)]


def _check(name, kind, got, tag, skip=()):
    """Every output of the reference, every element; every `*_ok` flag (floats that must keep their bits)."""
    _, r64, e32 = _reference(name, kind)
    bad = []
    for k, ref in r64.items():
        if k in skip:
            continue
        assert k in got, f"{name}: output {k} missing"
        assert got[k].shape == ref.shape, f"{name} {k}: shape {got[k].shape} vs {ref.shape}"
        err, bar = sc.rel_err(got[k], ref), max(FLOOR, 3 * e32[k])
        if not np.isfinite(err):
            err = float("inf")
        parity_record(f"stem/{tag}{kind}_{name}", **{f"{k}_err": err, f"{k}_e32": e32[k], f"{k}_bar": bar})
        print(f"stem {tag}{kind}:{name} {k}: err {err:.3e} e32 {e32[k]:.3e} bar {bar:.3e}")
        if not err <= bar:
            bad.append(f"{k}: err {err:.3e} > bar {bar:.3e}")
    flags = [k for k in got if k.endswith("_ok")]
    assert flags, f"{name}: no sentinel flags"
    for k in flags:
        if not bool(got[k]):
            bad.append(f"{k}: floats outside the outputs changed")
    if "fin_nbt" in got and int(got["fin_nbt"][0]) != 6:                     # 5 before the call
        bad.append(f"num_batches_tracked {int(got['fin_nbt'][0])}, expected 6")
    assert not bad, f"{tag}{kind}:{name}: " + "; ".join(bad)


def _child(tmp_path_factory, key):
    """The cases of one switch in a fresh process (run once per session): {"fwd:NAME": [outputs of run 0, of run 1]}."""
    if key not in _CHILD:
        env, reps, names = {"gather": ({"LHN_DW_GATHER": "1"}, 1, [f"{k}:{n}" for n in GATHER_CASES for k in ("fwd", "bwd")]),
                            "det": ({"LHN_DETERMINISTIC": "1"}, 2, [f"{k}:{n}" for n in DET_CASES for k in ("fwd", "bwd")] +
                                    [f"fwd:{n}" for n in sc.OFFSET])}[key]
        out = str(tmp_path_factory.mktemp("stem") / f"{key}.npz")
        base = {k: v for k, v in os.environ.items() if k not in ("LHN_DW_GATHER", "LHN_DETERMINISTIC")}
        r = subprocess.run([sys.executable, os.path.join(HERE, "stem_cases.py"), out, str(reps)] + names, env=dict(base, **env),
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        res = dict(np.load(out))
        _CHILD[key] = {nm: [{k[len(f"{nm}/{rep}/"):]: v for k, v in res.items() if k.startswith(f"{nm}/{rep}/")} for rep in range(reps)]
                       for nm in names}
    return _CHILD[key]


@pytest.mark.parametrize("name", list(sc.CASES))
def test_stem_fwd_matches_float64(dev, name):
    g, r64, e32 = _reference(name, "fwd")
    got = sc.run(name, dev, g)
    _check(name, "fwd", got, "")
    if "fin" in sc.CASES[name]["flags"]:
        parity_record(f"stem/fwd_{name}", fused_equals_separate_finalize_bits=bool(got["sep_bits_equal"]))
        print(f"stem fwd:{name} fused finalize == separate lhn_bn_finalize, bit for bit: {bool(got['sep_bits_equal'])}")
        for k in ("scale", "shift", "mean", "invstd", "rmean", "rvar"):      # the separate launch meets the same bar
            err, bar = sc.rel_err(got[f"sep_{k}"], r64[f"fin_{k}"]), max(FLOOR, 3 * e32[f"fin_{k}"])
            assert err <= bar, f"{name} lhn_bn_finalize {k}: err {err:.3e} > bar {bar:.3e}"


@pytest.mark.parametrize("name", sc.BWD_CASES)
def test_stem_bwd_matches_float64(dev, name):
    _check(name, "bwd", sc.run(name, dev, _reference(name, "bwd")[0], kind="bwd"), "")


GATHER_CASES = [n for n in sc.CASES if n.startswith(("m3_", "m7_"))]


def test_stem_gather_switch(dev, tmp_path_factory):
    """LHN_DW_GATHER=1: every MFMA shape on the direct kernels, forward and backward.  Same float64 bar."""
    for n in GATHER_CASES:
        assert sc.kernel_of(n).endswith("_mfma") and sc.kernel_of(n, kind="bwd").endswith("_mfma")
        assert sc.kernel_of(n, gather=True) == "k_stem_fwd" and sc.kernel_of(n, gather=True, kind="bwd").startswith("k_stem_bwd<")
    res = _child(tmp_path_factory, "gather")
    for name in GATHER_CASES:
        for kind in ("fwd", "bwd"):
            _check(name, kind, res[f"{kind}:{name}"][0], "LHN_DW_GATHER/")


DET_CASES = ["m3_32", "m3_33x29", "m7_32", "m7_23x19", "d3_c64", "d7_c32"]


def test_stem_deterministic_bits(dev, tmp_path_factory):
    """LHN_DETERMINISTIC=1: the library reports 2 CUs, so every persistent grid walks several tiles per workgroup (the tile loop and
    the one-tile-ahead prefetch); two runs agree bit for bit, statistics and gradients included, and the first meets the bar."""
    res = _child(tmp_path_factory, "det")
    for name in DET_CASES:
        for kind in ("fwd", "bwd"):
            a, b = res[f"{kind}:{name}"]
            assert a and a.keys() == b.keys()
            for k in a:
                np.testing.assert_array_equal(a[k], b[k], err_msg=f"{kind}:{name} {k}")
            _check(name, kind, a, "deterministic/")


@pytest.mark.parametrize("name", sc.NOSTATS_TWICE)
def test_stem_fwd_repeats_bits(dev, name):
    """Without statistics the forward has no atomics: two calls give the same bits (and meet the bar)."""
    g = _reference(name, "fwd")[0]
    a, b = sc.run(name, dev, g, stats=False), sc.run(name, dev, g, stats=False)
    assert "stats_sum" not in a and "fin_scale" not in a
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{name} {k}")
    _check(name, "fwd", a, "nostats/", skip=[k for k in _reference(name, "fwd")[1] if k != "y"])


@pytest.mark.parametrize("mode", ["default", "deterministic"])
@pytest.mark.parametrize("name", list(sc.OFFSET))
def test_stem_statistics_large_mean(dev, tmp_path_factory, name, mode):
    """The image is 1000 + N(0,1) and every feature's weights sum to 1: |mean| / sigma > 300 at the output, sq/n - (sum/n)^2 cancels
    six digits.  The two MFMA forwards keep per-lane sums shifted by the lane's first value (kk): the batch variance from the folded
    statistics stays within 1e-3 of float64, the bar test_batchnorm_statistics_large_mean sets for the other convolutions at the
    same premise.  The direct kernel k_stem_fwd is left out: it keeps plain fp32 per-thread sums (no shift), and at test size each
    thread sees one or two pixels, so a test here could not tell its sums from shifted ones."""
    g = _reference(name, "fwd")[0]
    ratio, var64 = sc.offset_premise(name, g)
    assert ratio > 300, ratio                                    # the premise: mean >> sigma at every channel of the output
    got = sc.run(name, dev, g) if mode == "default" else _child(tmp_path_factory, "det")[f"fwd:{name}"][0]
    c = sc.OFFSET[name]
    cnt = c["n"] * sc.out_hw(c)[0] * sc.out_hw(c)[1]
    var = got["stats_sq"] / cnt - (got["stats_sum"] / cnt) ** 2
    err = float((np.abs(var - var64) / var64).max())
    parity_record(f"stem/{mode}/fwd_{name}", batch_variance_err=err, batch_variance_bar=1e-3, mean_over_sigma=ratio)
    print(f"stem {mode} fwd:{name} batch variance err {err:.3e} bar 1.0e-03 (|mean| / sigma >= {ratio:.0f})")
    assert err < 1e-3, (name, mode, err)
    assert bool(got["y_outside_ok"]) and bool(got["stats_pad_ok"])
    _check(name, "fwd", got, f"{mode}/", skip=("stats_sum", "stats_sq"))


@pytest.mark.parametrize("name", list(sc.REFUSE))
def test_stem_refuses(dev, name):
    """The LDS cases never reach the runtime: lhn_conv_stem_fwd refuses them on its arguments, before any launch."""
    c = sc.REFUSE[name]
    rc, untouched = sc.run(name, dev, kind=c["kind"], expect_fail=True)
    assert rc == 1 and c["refuse"] in sc._lib.lib().lhn_last_error().decode()      # the invalid-argument status, for the reason the case names
    assert untouched, f"{name}: a refused call wrote to its outputs"
