"""Direct C-ABI checks of the `mynet` attention MLP (lhn_att_mlp_fwd / lhn_att_mlp_bwd) and of the squeeze-and-excitation gate MLP
(lhn_se_mlp_fwd2 / lhn_se_mlp_bwd2 and their mode-0 wrappers):
1. every output and every saved row, per element, against a float64 torch reference whose backward is autograd's (bar per output:
   max(2e-5, 3 x the error of the same reference in float32 on the CPU));
2. sentinel floats behind and around every output keep their bits; `save` has exactly the size include/lhn.h states;
3. two runs give the same bits -- every output under LHN_DETERMINISTIC=1, every output written without atomics in default mode;
4. the wrappers equal the `2` entry points with mode 0 bit for bit;
5. calls outside the supported set are refused without writing.
tests/att_se_cases.py holds the cases and says which branch each one reaches."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import att_se_cases as ac
from conftest import parity_record

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = list(ac.CASES)
WRAPPED = "se_n3_c256_j64_view_pre"          # the mode-0 case that also runs through lhn_se_mlp_fwd / lhn_se_mlp_bwd

_REF, _CHILD = {}, {}


def _reference(name):
    """(inputs, float64 reference, float32-on-the-CPU error per output); computed once per case and shared."""
    if name not in _REF:
        g = ac.inputs(name)
        r64, r32 = ac.reference(name, g), ac.reference(name, g, torch.float32)
        _REF[name] = (g, r64, {k: ac.rel_err(r32[k], r64[k]) for k in r64})
    return _REF[name]


def _check(name, got, tag=""):
    """Every output of the reference, every element; every `*_ok` flag (floats that must keep their bits); num_batches_tracked."""
    _, r64, e32 = _reference(name)
    bad = []
    for k, ref in r64.items():
        assert k in got, f"{name}: output {k} missing"
        assert got[k].shape == ref.shape, f"{name} {k}: shape {got[k].shape} vs {ref.shape}"
        err = ac.rel_err(got[k], ref)
        if not np.isfinite(err):
            err = float("inf")
        bar = max(ac.FLOOR, 3 * e32[k])
        parity_record(f"att_se/{tag}{name}", **{f"{k}_err": err, f"{k}_e32": e32[k], f"{k}_bar": bar})
        print(f"att_se {tag}{name} {k}: err {err:.3e} e32 {e32[k]:.3e} bar {bar:.3e}")
        if not err <= bar:
            bad.append(f"{k}: err {err:.3e} > bar {bar:.3e}")
    flags = [k for k in got if k.endswith("_ok")]
    assert flags, f"{name}: no sentinel flags"
    for k in flags:
        if not bool(got[k]):
            bad.append(f"{k}: floats outside the outputs changed")
    for k in [k for k in got if k.endswith("nbt")]:                    # 5 before the call
        want = 6 if ac.has_bwd(name) else 5
        if int(got[k][0]) != want:
            bad.append(f"{k}: num_batches_tracked {int(got[k][0])}, expected {want}")
    assert (name in ac.ATT) == any(k.endswith("nbt") for k in got)
    if ac.CASES[name].get("zero"):                                     # what flows through a dead unit: exact zeros, not small numbers
        for what, v in ac.dead_parts(name, got).items():
            same = not np.any(v)
            parity_record(f"att_se/{tag}{name}", **{f"{what}_exact_zero": bool(same)})
            if not same:
                bad.append(f"{what}: not identically zero")
    assert not bad, f"{tag}{name}: " + "; ".join(bad)


@pytest.mark.parametrize("name", NAMES)
def test_matches_float64(dev, name):
    _check(name, ac.run(name, dev, _reference(name)[0]))


def _child(tmp_path_factory, key):
    """Every case in a fresh process under the environment of `key`, twice (run once per session): {case: [outputs of run 0, of run 1]}."""
    if key not in _CHILD:
        env = {"default": {}, "det": {"LHN_DETERMINISTIC": "1"}}[key]
        names = NAMES + [WRAPPED + "@wrapper"]
        out = str(tmp_path_factory.mktemp("att_se") / f"{key}.npz")
        base = {k: v for k, v in os.environ.items() if k != "LHN_DETERMINISTIC"}
        r = subprocess.run([sys.executable, os.path.join(HERE, "att_se_cases.py"), out, "2"] + names, env=dict(base, **env),
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        res = dict(np.load(out))
        _CHILD[key] = {nm: [{k[len(f"{nm}/{rep}/"):]: v for k, v in res.items() if k.startswith(f"{nm}/{rep}/")} for rep in range(2)]
                       for nm in names}
    return _CHILD[key]


def _same(a, b, what, skip=()):
    assert a and a.keys() == b.keys(), what
    for k in a:
        if k.split("_")[-1] in skip:
            continue
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, f"{what} {k}"
        assert a[k].tobytes() == b[k].tobytes(), f"{what} {k}: {int((a[k] != b[k]).sum())} elements differ"


@pytest.mark.parametrize("name", NAMES)
def test_deterministic_mode_repeats_every_bit(dev, tmp_path_factory, name):
    """LHN_DETERMINISTIC=1: k_att_bwd2 and k_se_bwd run as ONE workgroup that walks the samples in order."""
    a, b = _child(tmp_path_factory, "det")[name]
    _same(a, b, f"deterministic {name}: run 0 vs run 1")
    _check(name, a, "deterministic/")


@pytest.mark.parametrize("name", NAMES)
def test_default_mode_repeats_what_it_writes_without_atomics(dev, tmp_path_factory, name):
    """The split is the code's (att_se_cases.ATOMIC): k_att_bwd2 adds dbl and dwl, k_se_bwd adds db2, dw2, db1 and dw1 with float
    atomics from one workgroup per sample -- those only meet their bars, in both runs; the forward, dpool, dad, dgamma, dbeta, dw3
    and db3 have one writer per element and repeat their bits."""
    a, b = _child(tmp_path_factory, "default")[name]
    assert any(k.split("_")[-1] in ac.ATOMIC for k in a) == ac.has_bwd(name)
    _same(a, b, f"default {name}: run 0 vs run 1", skip=ac.ATOMIC)
    _check(name, a, "child/")
    _check(name, b, "child2/")


@pytest.mark.parametrize("key", ["default", "det"])
def test_stage_1_then_2_gives_the_bits_of_stage_0(dev, tmp_path_factory, key):
    res = _child(tmp_path_factory, key)
    _same(res["att_stage12_c64"][0], res["att_stage0_c64"][0], f"{key}: stage 1 + 2 vs stage 0", skip=() if key == "det" else ac.ATOMIC)


def test_wrappers_equal_mode_0(dev, tmp_path_factory):
    """lhn_se_mlp_fwd / lhn_se_mlp_bwd against lhn_se_mlp_fwd2 / lhn_se_mlp_bwd2 with mode 0, deterministic mode: every output."""
    res = _child(tmp_path_factory, "det")
    assert ac.SE[WRAPPED]["m"] == 0
    _same(res[WRAPPED + "@wrapper"][0], res[WRAPPED][0], "wrapper vs mode 0")


@pytest.mark.parametrize("name", list(ac.REFUSE))
def test_refuses_without_writing(dev, name):
    rc, untouched, err = ac.refuse(name, dev)
    assert rc == 1 and ac.REFUSE[name][2] in err, (rc, err)      # the invalid-argument status, for the reason the case names
    assert untouched, f"{name}: a refused call wrote to its outputs"
