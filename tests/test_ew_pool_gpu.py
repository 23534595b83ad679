"""Direct C-ABI checks of everything that sits between two convolutions of a plan, per element against a float64 torch reference:
the elementwise combine k_ew_fwd<BIL> (sum, product, nearest and bilinear resampling, coefficients, SiLU / ReLU-sigmoid) and its
backward forms (k_ew_bwd_src, k_ew_bwd_multi, k_ew_mul_bwd, k_bilinear_bwd), channel shuffle, the 2x2 ceil-mode max pool with its
BatchNorm-sum and gradient-addend variants, the adaptive average pool (small and workgroup kernels, STAT and COPY forms, backward)
and the gate-gradient reduce.  Outputs that are pure moves must match the float32 reference bit for bit, deterministic mode must
repeat its bits over grids that iterate, and calls outside the supported set are refused without writing.
profiles/ew_pool_instances.md lists which case reaches which kernel, instance and path."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ew_pool_cases as ec
from conftest import parity_record

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FLOOR = 2e-5        # the project's kernel-level floor (test_pw_gpu.FLOOR)

_REF = {}


def _reference(group, name):
    """(inputs, float64 reference, float32 reference, float32-on-the-CPU error per output); computed once per case and shared."""
    if (group, name) not in _REF:
        g = ec.inputs(group, name)
        r64, r32 = ec.reference(group, name, g), ec.reference(group, name, g, torch.float32)
        _REF[(group, name)] = (g, r64, r32, {k: ec.rel_err(r32[k], r64[k]) for k in r64})
    return _REF[(group, name)]


def _check(group, name, got, tag=""):
    """Every output of the reference, every element; every `*_ok` flag (floats that must keep their bits)."""
    _, r64, r32, e32 = _reference(group, name)
    bad = []
    for k, ref in r64.items():
        assert k in got, f"{group}:{name}: output {k} missing"
        assert got[k].shape == ref.shape, f"{group}:{name} {k}: shape {got[k].shape} vs {ref.shape}"
        err = ec.rel_err(got[k], ref)
        if not np.isfinite(err):
            err = float("inf")
        if k in ec.exact_keys(group, name):      # floats moved (or added once): the float32 reference's bits
            same = np.array_equal(got[k], r32[k].astype(np.float32))
            parity_record(f"ew_pool/{tag}{group}_{name}", **{f"{k}_err": err, f"{k}_bits_equal": bool(same)})
            print(f"ew_pool {tag}{group}:{name} {k}: err {err:.3e} bit-equal {same}")
            if not same:
                bad.append(f"{k}: differs from the float32 reference in some bit (err {err:.3e})")
            continue
        bar = max(FLOOR, 3 * e32[k])
        parity_record(f"ew_pool/{tag}{group}_{name}", **{f"{k}_err": err, f"{k}_e32": e32[k], f"{k}_bar": bar})
        print(f"ew_pool {tag}{group}:{name} {k}: err {err:.3e} e32 {e32[k]:.3e} bar {bar:.3e}")
        if not err <= bar:
            bad.append(f"{k}: err {err:.3e} > bar {bar:.3e}")
    flags = [k for k in got if k.endswith("_ok")]
    assert flags, f"{group}:{name}: no sentinel flags"
    for k in flags:
        if not bool(got[k]):
            bad.append(f"{k}: floats outside the outputs changed")
    assert not bad, f"{tag}{group}:{name}: " + "; ".join(bad)


def _cases(group):
    return list(ec.GROUPS[group])


@pytest.mark.parametrize("name", _cases("ewf"))
def test_combine_forward_matches_float64(dev, name):
    _check("ewf", name, ec.run("ewf", name, dev, _reference("ewf", name)[0]))


@pytest.mark.parametrize("name", _cases("ewb"))
def test_combine_backward_matches_float64(dev, name):
    _check("ewb", name, ec.run("ewb", name, dev, _reference("ewb", name)[0]))


@pytest.mark.parametrize("name", _cases("mul"))
def test_product_backward_matches_float64(dev, name):
    _check("mul", name, ec.run("mul", name, dev, _reference("mul", name)[0]))


@pytest.mark.parametrize("name", _cases("bil"))
def test_bilinear_backward_matches_float64(dev, name):
    _check("bil", name, ec.run("bil", name, dev, _reference("bil", name)[0]))


@pytest.mark.parametrize("group,name", [(g, n) for g in ("shf", "shb") for n in _cases(g)])
def test_shuffle_matches_float64(dev, group, name):
    _check(group, name, ec.run(group, name, dev, _reference(group, name)[0]))


@pytest.mark.parametrize("name", _cases("mp"))
def test_maxpool_matches_float64(dev, name):
    _check("mp", name, ec.run("mp", name, dev, _reference("mp", name)[0]))


@pytest.mark.parametrize("group,name", [(g, n) for g in ("apf", "apb") for n in _cases(g)])
def test_avgpool_matches_float64(dev, group, name):
    _check(group, name, ec.run(group, name, dev, _reference(group, name)[0]))


@pytest.mark.parametrize("name", _cases("gate"))
def test_gate_reduce_matches_float64(dev, name):
    _check("gate", name, ec.run("gate", name, dev, _reference("gate", name)[0]))


def test_deterministic_bits(dev, tmp_path):
    """LHN_DETERMINISTIC=1: the library reports 2 CUs, so the row grids cap at 16 workgroups and their loops iterate (every case here
    has more rows than that); two runs agree bit for bit, the BatchNorm sums and the gate sums included, and meet the bar."""
    for full in ec.DET:
        grp, nm = full.split(":")
        assert ec.rows(grp, nm) > 16, f"{full}: {ec.rows(grp, nm)} rows"
    out = str(tmp_path / "out.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "ew_pool_cases.py"), out, "2"] + ec.DET, env=dict(os.environ, LHN_DETERMINISTIC="1"),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = dict(np.load(out))
    for full in ec.DET:
        grp, nm = full.split(":")
        a, b = ({k[len(f"{full}/{rep}/"):]: v for k, v in res.items() if k.startswith(f"{full}/{rep}/")} for rep in (0, 1))
        assert a and a.keys() == b.keys()
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{full} {k}")
        _check(grp, nm, a, "deterministic/")


@pytest.mark.parametrize("key", list(ec.REFUSE))
def test_refuses(dev, key):
    group, name, case, text = ec.REFUSE[key]
    rc, untouched = ec.run(group, name, dev, ec.refuse_inputs(key), expect_fail=True, case=case)
    err = ec._lib.lib().lhn_last_error().decode()
    assert rc != 0 and text in err, f"{key}: status {rc}, error {err!r}"            # refused for the reason the case names
    assert untouched, f"{key}: a refused call wrote to its outputs"
