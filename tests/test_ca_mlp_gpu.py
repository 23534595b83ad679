"""Direct C-ABI checks of the channel-attention MLP, lhn_ca_mlp_fwd and lhn_ca_mlp_bwd2:
1. every output, per element, against a float64 torch reference (bar per output: max(2e-5, 3 x the error of the same reference in
   float32 on the CPU); sentinel floats around every output keep their bits);
2. the staged kernels (default) against the four they replace (LHN_CA_MLP_V1=1): every output bit for bit, each setting in a fresh
   process, and one small training step end to end;
3. two runs in one process give the same bits, in default and in deterministic mode.
tests/ca_mlp_cases.py holds the cases and says which branch each one reaches."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ca_mlp_cases as cc
from conftest import parity_record

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = list(cc.CASES)

_REF, _CHILD = {}, {}


def _reference(name):
    """(inputs, float64 reference, float32-on-the-CPU error per output); computed once per case and shared."""
    if name not in _REF:
        g = cc.inputs(name)
        r64, r32 = cc.reference(name, g), cc.reference(name, g, torch.float32)
        _REF[name] = (g, r64, {k: cc.rel_err(r32[k], r64[k]) for k in r64})
    return _REF[name]


def _check(name, got, tag=""):
    _, r64, e32 = _reference(name)
    c, bad = cc.CASES[name], []
    for k, ref in r64.items():
        assert k in got, f"{name}: output {k} missing"
        assert got[k].shape == ref.shape, f"{name} {k}: shape {got[k].shape} vs {ref.shape}"
        if c.get("zero_bwd") and not np.abs(ref).max() > 0:          # N = 1: exact zeros, not small numbers
            same = not np.any(got[k])
            parity_record(f"ca_mlp/{tag}{name}", **{f"{k}_exact_zero": bool(same)})
            print(f"ca_mlp {tag}{name} {k}: exact zeros {same}")
            if not same:
                bad.append(f"{k}: not identically zero")
            continue
        err = cc.rel_err(got[k], ref)
        if not np.isfinite(err):
            err = float("inf")
        bar = max(cc.FLOOR, 3 * e32[k])
        parity_record(f"ca_mlp/{tag}{name}", **{f"{k}_err": err, f"{k}_e32": e32[k], f"{k}_bar": bar})
        print(f"ca_mlp {tag}{name} {k}: err {err:.3e} e32 {e32[k]:.3e} bar {bar:.3e}")
        if not err <= bar:
            bad.append(f"{k}: err {err:.3e} > bar {bar:.3e}")
    flags = [k for k in got if k.endswith("_ok")]
    assert flags, f"{name}: no sentinel flags"
    for k in flags:
        if not bool(got[k]):
            bad.append(f"{k}: floats outside the outputs changed")
    want = 5 + (1 if cc.mode(name) == "train" else 0)
    if int(got["nbt"][0]) != want:
        bad.append(f"num_batches_tracked {int(got['nbt'][0])}, expected {want}")
    assert not bad, f"{tag}{name}: " + "; ".join(bad)


@pytest.mark.parametrize("name", NAMES)
def test_matches_float64(dev, name):
    _check(name, cc.run(name, dev, _reference(name)[0]))


def _child(tmp_path_factory, key):
    """Every case in a fresh process under the environment of `key` (run once per session): {case: [outputs of run 0, of run 1]}."""
    if key not in _CHILD:
        env, reps = {"default": ({}, 2), "v1": ({"LHN_CA_MLP_V1": "1"}, 1), "det": ({"LHN_DETERMINISTIC": "1"}, 2)}[key]
        out = str(tmp_path_factory.mktemp("ca_mlp") / f"{key}.npz")
        base = {k: v for k, v in os.environ.items() if k not in ("LHN_CA_MLP_V1", "LHN_DETERMINISTIC")}
        r = subprocess.run([sys.executable, os.path.join(HERE, "ca_mlp_cases.py"), out, str(reps)] + NAMES, env=dict(base, **env),
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        res = dict(np.load(out))
        _CHILD[key] = {nm: [{k[len(f"{nm}/{rep}/"):]: v for k, v in res.items() if k.startswith(f"{nm}/{rep}/")} for rep in range(reps)]
                       for nm in NAMES}
    return _CHILD[key]


def _same(a, b, what):
    assert a and a.keys() == b.keys(), what
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, f"{what} {k}"
        assert a[k].tobytes() == b[k].tobytes(), f"{what} {k}: {int((a[k] != b[k]).sum())} elements differ"


@pytest.mark.parametrize("name", NAMES)
def test_staged_kernels_keep_the_bits_of_the_old_ones(dev, tmp_path_factory, name):
    new, old = _child(tmp_path_factory, "default")[name][0], _child(tmp_path_factory, "v1")[name][0]
    _same(new, old, f"{name}: default vs LHN_CA_MLP_V1=1")
    _check(name, old, "v1/")


@pytest.mark.parametrize("key", ["default", "v1", "det"])
def test_stage_1_then_2_gives_the_bits_of_stage_0(dev, tmp_path_factory, key):
    res = _child(tmp_path_factory, key)
    _same(res["stage12_c64"][0], res["stage0_c64"][0], f"{key}: stage 1 + 2 vs stage 0")


@pytest.mark.parametrize("key", ["default", "det"])
def test_two_runs_give_the_same_bits(dev, tmp_path_factory, key):
    res = _child(tmp_path_factory, key)
    for name in NAMES:
        _same(res[name][0], res[name][1], f"{key} {name}: run 0 vs run 1")
        if key == "det":
            _check(name, res[name][0], "deterministic/")


def test_train_step_is_bit_identical_with_and_without_the_switch(dev, tmp_path):
    """One MSRB and one gated RepBasicUnit (batch 4, 16 x 16 map, dropout live), deterministic mode: loss, gradients, buffers."""
    res = []
    for mode in ("0", "1"):
        out = str(tmp_path / f"camlp{mode}.npz")
        r = subprocess.run([sys.executable, os.path.join(HERE, "ca_mlp_cases.py"), "--train-step", out],
                           env=dict(os.environ, LHN_CA_MLP_V1=mode, LHN_DETERMINISTIC="1"), capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        res.append(np.load(out))
    a, b = res
    assert set(a.files) == set(b.files) and any(k.startswith("g.") for k in a.files) and any(k.startswith("b.") for k in a.files)
    assert np.isfinite(a["loss"]) and float(np.abs(a["gflat"]).max()) > 0
    assert any("ca" in k and k.startswith("g.") and float(np.abs(a[k]).max()) > 0 for k in a.files), "no attention gradient"
    for k in a.files:
        assert a[k].tobytes() == b[k].tobytes(), k
