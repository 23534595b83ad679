"""The stem convolution with 40 output channels (3 -> 40, k = 3, stride 2: the first convolution of mynet at width 160) through the C
ABI, per element against float64 with the bars of tests/test_stem_gpu.py: max(2e-5, 3 * e32) per output, every `*_ok` guard, the
fused BatchNorm finalize bit for bit against a separate lhn_bn_finalize, the weight gradient over replicas (folded on the host and by
lhn_reduce_replicas), deterministic mode twice with the same bits.  tests/stem40_cases.py lists the cases.  On a library without
the 40-channel admission every case stops with `Cout=40`; Cout = 24 stays refused."""
import os
import subprocess
import sys

import numpy as np
import pytest

import stem40_cases as s4
import stem_cases as sc
from conftest import parity_record
from test_stem_gpu import FLOOR, _check, _reference

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("name", list(s4.CASES))
def test_stem40_fwd_matches_float64(dev, name):
    g, r64, e32 = _reference(name, "fwd")
    got = sc.run(name, dev, g)
    _check(name, "fwd", got, "w160/")
    if "fin" in s4.CASES[name]["flags"]:
        parity_record(f"stem/w160/fwd_{name}", fused_equals_separate_finalize_bits=bool(got["sep_bits_equal"]))
        assert bool(got["sep_bits_equal"]), f"{name}: the fused finalize and lhn_bn_finalize disagree"
        for k in ("scale", "shift", "mean", "invstd", "rmean", "rvar"):
            err, bar = sc.rel_err(got[f"sep_{k}"], r64[f"fin_{k}"]), max(FLOOR, 3 * e32[f"fin_{k}"])
            assert err <= bar, f"{name} lhn_bn_finalize {k}: err {err:.3e} > bar {bar:.3e}"


@pytest.mark.parametrize("name", list(s4.CASES))
def test_stem40_bwd_matches_float64(dev, name):
    _check(name, "bwd", sc.run(name, dev, _reference(name, "bwd")[0], kind="bwd"), "w160/")


def test_stem40_fwd_without_statistics_repeats_bits(dev):
    name = "c40_concat"
    g = _reference(name, "fwd")[0]
    a, b = sc.run(name, dev, g, stats=False), sc.run(name, dev, g, stats=False)
    assert "stats_sum" not in a and "fin_scale" not in a
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{name} {k}")
    _check(name, "fwd", a, "w160/nostats/", skip=[k for k in _reference(name, "fwd")[1] if k != "y"])


def test_stem40_deterministic_bits(dev, tmp_path):
    """LHN_DETERMINISTIC=1 (2 CUs: every block walks several rounds of pixels): two runs agree bit for bit and meet the bar."""
    names = [f"{k}:{n}" for n in ("c40_odd", "c40_concat") for k in ("fwd", "bwd")]
    out = str(tmp_path / "det.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("LHN_DW_GATHER", "LHN_DETERMINISTIC")}
    r = subprocess.run([sys.executable, os.path.join(HERE, "stem40_cases.py"), out, "2"] + names, env=dict(env, LHN_DETERMINISTIC="1"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = dict(np.load(out))
    for full in names:
        kind, name = full.split(":")
        a, b = ({k[len(f"{full}/{rep}/"):]: v for k, v in res.items() if k.startswith(f"{full}/{rep}/")} for rep in (0, 1))
        assert a and a.keys() == b.keys()
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{full} {k}")
        _check(name, kind, a, "w160/deterministic/")


@pytest.mark.parametrize("name", list(s4.REFUSE))
def test_stem40_refuses(dev, name):
    c = s4.REFUSE[name]
    rc, untouched = sc.run(name, dev, kind=c["kind"], expect_fail=True)
    assert rc == 1 and c["refuse"] in sc._lib.lib().lhn_last_error().decode()
    assert untouched, f"{name}: a refused call wrote to its outputs"
