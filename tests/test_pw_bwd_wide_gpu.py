"""The register-W backward of the wide 1x1 convolutions (k_pw_bwd_wr: 128 -> 128, 64 -> 128, 128 -> 64), called through
lhn_conv_pw_bwd3 and compared element by element (dx, dW, dbias, and the dy left in dz) with a float64 computation on the CPU.
Inputs, the kernel call and the reference are those of tests/pw_cases.py; the cases below are added to its table in memory.

Bar: the split path (k_dy_inplace + dgrad + wgrad: the code before this kernel, reached with LHN_PW_BWD_SPLIT=1 in a child
process) runs the same cases in the same session; for each output the new kernel's largest error against float64, relative to
the output's largest magnitude, may be at most twice the split path's: another fp32 summation order over the same terms.

dz: lhn_pw_bwd_split overwrites dz with dy, and tests/test_pw_gpu.py pins that for these shapes on the default path, so the new
kernel stores dy over dz as well and the check here is that dz holds dy (same bar) and that no float outside the view changed.

Measured (profiles/parity_pw_bwd_wide.json, 25 entries): errors of 6e-8 .. 4e-7 on both paths; the largest ratio new / split is
1.67 (dbias of the 9-pixel cases: nine terms in another order); dx and dz have the same error as the split path in every case.

Run as a script it is the child: python tests/test_pw_bwd_wide_gpu.py OUT.npz REPEATS NAME ..."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pw_cases as pc
from conftest import parity_record

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FACTOR = 2.0
PAIRS = ((128, 128), (64, 128), (128, 64))
# pixel counts: 70 = one 64-pixel tile (two of 32) and a 6-row tail; 9 = under one tile; 192 = three tiles of 64 / six of 32
PIXELS = {"tail": (2, 5, 7), "tiny": (1, 3, 3), "tiles": (3, 8, 8)}

CASES = {}
for _ci, _co in PAIRS:
    for _tag, _nhw in PIXELS.items():
        CASES[f"wide_{_ci}_{_co}_{_tag}"] = pc._case(_ci, _co, _nhw, "split dbias")
    # 320 pixels = five tiles of 64: more tiles than the four workgroups of deterministic mode, for the 64-pixel instances too
    CASES[f"wide_{_ci}_{_co}_loop"] = pc._case(_ci, _co, (5, 8, 8), "split")
# variations on 128 -> 128 at 70 pixels (always: pending table with leaky slope 0.1 on x and y, non-trivial A | B | C, dx prefilled)
for _nm, _fl, _kw in (("store", "split", {}),                        # dx_accumulate = 0 into a dx that holds 7.0
                      ("acc", "split acc", {}),                      # dx_accumulate = 1 into a random prior
                      ("nodx", "split nodx", {}),                    # dx = NULL
                      ("nrep1", "split dbias acc", {"nrep": 1}),     # one gradient replica (the base cases: four, dbias present)
                      ("xgate", "split xgate", {}),
                      ("views", "split views dbias", {}),            # x / dx at channel 64, y / dz at channel 32 of wider buffers
                      ("ygate_dpool", "split ygate dpool", {})):     # the terms of lhn_grad_du that need pixel coordinates
    CASES[f"wide_128_128_{_nm}"] = pc._case(128, 128, PIXELS["tail"], _fl, **_kw)
pc._ALL["bwd"].update(CASES)          # (not pc.BWD: tests/test_pw_gpu.py parametrises over that)
DET_CASES = [n for n in CASES if n.endswith(("_tiles", "_loop"))]
OUTPUTS = ("dx", "dw", "dbias", "dz")

_REF = {}


def _reference(name):
    if name not in _REF:
        g = pc.inputs("bwd", name)
        _REF[name] = (g, pc.reference_bwd(name, g))
    return _REF[name]


def _child(tmp, env_extra, names, reps):
    out = os.path.join(str(tmp), "out.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out, str(reps)] + names, env=dict(os.environ, **env_extra),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return dict(np.load(out))


def _of(res, name, rep):
    pre = f"{name}/{rep}/"
    return {k[len(pre):]: v for k, v in res.items() if k.startswith(pre)}


@pytest.fixture(scope="module")
def split_runs(dev, tmp_path_factory):
    """Every case on the split path, once per session."""
    return _child(tmp_path_factory.mktemp("pw_bwd_split"), {"LHN_PW_BWD_SPLIT": "1"}, list(CASES), 1)


def _compare(name, got, old, tag=""):
    """Every output of the float64 reference, every element: new error <= FACTOR x the split path's error on the same case."""
    _, r64 = _reference(name)
    bad = []
    for k in OUTPUTS:
        if k not in r64:      # (dx = NULL, no dbias)
            continue
        assert got[k].shape == r64[k].shape == old[k].shape, f"{name} {k}: shapes {got[k].shape} {old[k].shape} {r64[k].shape}"
        e_new, e_old = pc.rel_err(got[k], r64[k]), pc.rel_err(old[k], r64[k])
        if not np.isfinite(e_new):
            e_new = float("inf")
        parity_record(f"pw_bwd_wide/{tag}{name}", **{f"{k}_err_wr": e_new, f"{k}_err_split": e_old, f"{k}_bar": FACTOR * e_old})
        print(f"pw_bwd_wide {tag}{name} {k}: k_pw_bwd_wr {e_new:.3e}  split {e_old:.3e}  bar {FACTOR * e_old:.3e}")
        if not e_new <= FACTOR * e_old:
            bad.append(f"{k}: {e_new:.3e} > {FACTOR} x {e_old:.3e}")
    for k, v in got.items():
        if k.endswith("_ok") and not bool(v):
            bad.append(f"{k}: floats outside the outputs changed")
    assert not bad, f"{tag}{name}: " + "; ".join(bad)


@pytest.mark.parametrize("name", list(CASES))
def test_pw_bwd_wide_matches_float64(dev, split_runs, name):
    g, r64 = _reference(name)
    got = pc.run_bwd(name, dev, g)
    c = CASES[name]
    assert ("dx" in got) == ("nodx" not in c["flags"]) and ("dbias" in got) == ("dbias" in c["flags"])
    _compare(name, got, _of(split_runs, name, 0))


def test_pw_bwd_wide_deterministic(dev, tmp_path):
    """LHN_DETERMINISTIC=1: four workgroups, so a workgroup walks more than one tile; two runs agree bit for bit and meet the
    bar against the split path under the same switch."""
    new = _child(tmp_path, {"LHN_DETERMINISTIC": "1"}, DET_CASES, 2)
    old_dir = tmp_path / "split"
    old_dir.mkdir()
    old = _child(old_dir, {"LHN_DETERMINISTIC": "1", "LHN_PW_BWD_SPLIT": "1"}, DET_CASES, 1)
    for name in DET_CASES:
        a, b = _of(new, name, 0), _of(new, name, 1)
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{name} {k}")
        _compare(name, a, _of(old, name, 0), "deterministic/")


def test_pw_bwd_split_switch_takes_the_old_path(dev, split_runs):
    """LHN_PW_BWD_SPLIT=1: the three-launch path still answers (the float64 bar of tests/test_pw_gpu.py), and it is another
    kernel than the default.  128 -> 128 sums dW over 32-pixel tiles where k_kxk_wgrad takes 64, so 70 pixels arrive as
    32 + 32 + 6 against 64 + 6 and the bits of dW differ; the 64-pixel instances add the same terms in the same order as the
    split path (equal bits are possible there and say nothing)."""
    import torch
    for name in ("wide_128_128_tail", "wide_64_128_tail", "wide_128_64_tail"):
        g, r64 = _reference(name)
        r32 = pc.reference_bwd(name, g, torch.float32)
        old = _of(split_runs, name, 0)
        for k, ref in r64.items():
            bar = max(2e-5, 3 * pc.rel_err(r32[k], ref))
            assert pc.rel_err(old[k], ref) <= bar, f"LHN_PW_BWD_SPLIT=1 {name} {k}"
        assert all(bool(v) for k, v in old.items() if k.endswith("_ok")), name
        if name == "wide_128_128_tail":
            got = pc.run_bwd(name, dev, g)
            assert not np.array_equal(got["dw"], old["dw"]), f"{name}: the switch did not change the kernel"


if __name__ == "__main__":
    import torch
    dst, reps, names = sys.argv[1], int(sys.argv[2]), sys.argv[3:]
    device = torch.device("cuda:0")
    res = {}
    for nm in names:
        inp = pc.inputs("bwd", nm)
        for rep in range(reps):
            for key, val in pc.run_bwd(nm, device, inp).items():
                res[f"{nm}/{rep}/{key}"] = val
    np.savez(dst, **res)
