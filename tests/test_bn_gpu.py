"""Direct C-ABI checks of the kernels between a convolution and its BatchNorm on the way back, per element against a float64
reference: lhn_bn_bwd_reduce (both reductions, dead pixel lanes, the four-pixel pass with clamped tail loads, the pooled-gradient
lookup) with and without its fused finalize, lhn_bn_finalize2 and lhn_bn_bwd_finalize2 at every replica grouping and in the second
round of their channel loops, lhn_fold_stat_replicas and lhn_reduce_replicas bit for bit against a sequential host sum.
Deterministic mode must repeat the reduction's bits, and calls outside the supported set are refused without writing.
tests/bn_cases.py holds the cases and says which branch each one reaches."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bn_cases as bc
from conftest import parity_record

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FLOOR = 2e-5        # the project's kernel-level floor (test_pw_gpu.FLOOR)

_REF = {}


def _reference(name):
    """(inputs, float64 reference, float32-on-the-CPU error per output); computed once per case and shared."""
    if name not in _REF:
        g = bc.inputs(name)
        r64, r32 = bc.reference(name, g), bc.reference(name, g, torch.float32)
        _REF[name] = (g, r64, {k: bc.rel_err(r32[k], r64[k]) for k in r64})
    return _REF[name]


def _check(name, got, tag):
    """Every output of the reference, every element; every `*_ok` flag (floats that must keep their bits)."""
    _, r64, e32 = _reference(name)
    bad = []
    for k, ref in r64.items():
        assert k in got, f"{name}: output {k} missing"
        assert got[k].shape == ref.shape, f"{name} {k}: shape {got[k].shape} vs {ref.shape}"
        err, bar = bc.rel_err(got[k], ref), max(FLOOR, 3 * e32[k])
        if not np.isfinite(err):
            err = float("inf")
        parity_record(f"bn/{tag}{name}", **{f"{k}_err": err, f"{k}_e32": e32[k], f"{k}_bar": bar})
        print(f"bn {tag}{name} {k}: err {err:.3e} e32 {e32[k]:.3e} bar {bar:.3e}")
        if not err <= bar:
            bad.append(f"{k}: err {err:.3e} > bar {bar:.3e}")
    flags = [k for k in got if k.endswith("_ok")]
    assert flags, f"{name}: no sentinel flags"
    for k in flags:
        if not bool(got[k]):
            bad.append(f"{k}: floats outside the outputs changed")
    assert not bad, f"{tag}{name}: " + "; ".join(bad)


@pytest.mark.parametrize("name", list(bc.CASES))
def test_bn_matches_float64(dev, name):
    g, r64, e32 = _reference(name)
    c, got = bc.CASES[name], bc.run(name, dev, g)
    _check(name, got, "")
    if name in bc.FUSED_CASES:
        parity_record(f"bn/{name}", fused_equals_separate_finalize_bits=bool(got["sep_bits_equal"]))      # (they fold the replicas in different orders)
        print(f"bn {name} fused finalize == separate lhn_bn_bwd_finalize2, bit for bit: {bool(got['sep_bits_equal'])}")
        for k in ("coef_A", "coef_B", "coef_C", "dgamma", "dbeta"):          # the separate launch meets the same bar
            err, bar = bc.rel_err(got[f"sep_{k}"], r64[k]), max(FLOOR, 3 * e32[k])
            assert err <= bar, f"{name} lhn_bn_bwd_finalize2 {k}: err {err:.3e} > bar {bar:.3e}"
    if c["op"] == "finalize":
        assert int(got["nbt"][0]) == (5 if "eval" in c["flags"] else 6)      # 5 before the call
    if c["op"] in ("fold", "repl"):                                          # the replicas in order r = 0, 1, ..: the host's bits
        k, want = ("rep0" if c["op"] == "fold" else "out"), bc.exact(name, g)
        assert got[k].dtype == want.dtype and got[k].tobytes() == want.tobytes(), \
            f"{name}: {int((got[k] != want).sum())} of {want.size} elements differ from the sequential host sum"


def test_bn_reduce_deterministic_bits(dev, tmp_path):
    """LHN_DETERMINISTIC=1: the library reports 2 CUs (16 workgroups, each with a statistics replica of its own, looping over rows);
    two runs of every reduce case, fused finalize included, agree bit for bit, and the first meets the bar."""
    names = bc.REDUCE_CASES + bc.FUSED_CASES
    out = str(tmp_path / "det.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "bn_cases.py"), out, "2"] + names, env=dict(os.environ, LHN_DETERMINISTIC="1"),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = dict(np.load(out))
    for name in names:
        a, b = ({k[len(f"{name}/{rep}/"):]: v for k, v in res.items() if k.startswith(f"{name}/{rep}/")} for rep in range(2))
        assert a and a.keys() == b.keys()
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{name} {k}")
        _check(name, a, "deterministic/")


@pytest.mark.parametrize("name", list(bc.REFUSE))
def test_bn_refuses(dev, name):
    rc, untouched = bc.run(name, dev, expect_fail=True)
    assert rc == 1 and bc.REFUSE[name]["refuse"] in bc._lib.lib().lhn_last_error().decode()      # the invalid-argument status, for the reason the case names
    assert untouched, f"{name}: a refused call wrote to its outputs"
