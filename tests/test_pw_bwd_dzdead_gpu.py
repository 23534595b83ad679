"""lhn_conv_pw_bwd6 with LHN_PW_BWD_DZ_DEAD (include/lhn.h): the wide register-W backward of the 1x1 convolution (k_pw_bwd_wr:
128 -> 128, 64 -> 128, 128 -> 64) without its dy store, through the C ABI, and the plan executor's use of the flag end to end.

Shapes: 128 -> 128 at 3 x 5 x 7 = 105 pixels (three 32-pixel tiles and a ragged fourth of 9), 64 -> 128 and 128 -> 64 at
2 x 9 x 9 = 162 pixels (two 64-pixel tiles and a ragged third of 34); each with dbias, with dx accumulated, with the BatchNorm-backward
finalize source (lhn_bnbwdsrc: the prologue fold), with both; 128 -> 128 also on channel-slice views with gates and pooled gradient.
Inputs and the float64 reference are those of tests/pw_cases.py, the finalize inputs those of tests/test_bwd_fin_consumer_gpu.py (the
reference takes the coefficients a separate lhn_bn_bwd_finalize2 launch wrote, and the fold's must equal them bit for bit).

Bar (that of tests/test_pw_bwd_wide_gpu.py): the split path (LHN_PW_BWD_SPLIT=1, a child process) runs the same cases; for dx, dW and
dbias the largest error against float64, relative to the output's largest magnitude, may be at most twice the split path's.
dz: after a call with the flag the whole dz buffer holds the bits it held before; no float outside the views changes.
LHN_DETERMINISTIC=1 (a child process): lhn_conv_pw_bwd6 with the flag and lhn_conv_pw_bwd5 agree bit for bit in dx, dW, dbias, the
coefficients, dgamma and dbeta.

End to end (a child process per setting, LHN_DETERMINISTIC=1): one train step of MSRB(128) -> RepBasicUnit(128) at N = 2, 16 x 16 and
of variant B at N = 2, 64 x 64: loss, every gradient and every buffer bit-identical with LHN_PW_BWD_DY_STORE=1 and without it.
(Which ops of these plans take the flag: tests/test_pw_dzdead_plan_cpu.py.)

Run as a script it is the child: python tests/test_pw_bwd_dzdead_gpu.py OUT.npz NAME ..."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pw_cases as pc
from litehandnet_amd import _lib
from litehandnet_amd._lib import GradView
from test_bwd_fin_consumer_gpu import FILL, _bn_inputs, _on, _same_bits, _separate, _src

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FACTOR = 2.0
DZ_DEAD = 1         # LHN_PW_BWD_DZ_DEAD
PIXELS = {(128, 128): (3, 5, 7), (64, 128): (2, 9, 9), (128, 64): (2, 9, 9)}

# name: (pw_cases case, BatchNorm extras of the finalize source or None)
CASES = {}
for (_ci, _co), _nhw in PIXELS.items():
    CASES[f"{_ci}_{_co}_dbias"] = (pc._case(_ci, _co, _nhw, "dbias"), None)
    CASES[f"{_ci}_{_co}_acc"] = (pc._case(_ci, _co, _nhw, "acc"), None)
    CASES[f"{_ci}_{_co}_fin"] = (pc._case(_ci, _co, _nhw, ""), {})
    CASES[f"{_ci}_{_co}_fin_acc_dbias"] = (pc._case(_ci, _co, _nhw, "acc dbias"), {"prior": True, "pscale": 0.5})
CASES["128_128_views_fin"] = (pc._case(128, 128, PIXELS[(128, 128)], "xgate ygate dpool dbias views"), {"sc": 136, "nogamma": True})
for _n, (_c, _) in CASES.items():
    pc._ALL["bwd"]["dzdead_" + _n] = _c
OUTPUTS = ("dx", "dw", "dbias")


def _bn(case):
    name, extras = "dzdead_" + case, CASES[case][1]
    if extras is None:
        return None
    c = pc._ALL["bwd"][name]
    (n, _, _), (_, _, _, _, ho, wo) = c["nhw"], pc.geometry("bwd", name)
    return _bn_inputs(c["cout"], n * ho * wo, extras, 13)


def _run(case, dev, g, entry, flags, bn):
    """One call of lhn_conv_pw_bwd5 (entry 5) or lhn_conv_pw_bwd6 (entry 6, with flags) on the case's inputs; bn: the finalize source's
    inputs on the device (consumed: dgamma and dbeta are written) or None, then g["coef"] is the table."""
    name = "dzdead_" + case
    c = pc._ALL["bwd"][name]
    f, (n, h, w), cin, cout = c["flags"], c["nhw"], c["cin"], c["cout"]
    xcs, xcoff, ycs, ycoff, ho, wo = pc.geometry("bwd", name)
    d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in g.items()}
    vx = pc._view(d["x"], xcoff, cin, d["xtab"], d.get("xgate"))
    vy = pc._view(d["y"], ycoff, cout, d["ytab"], d.get("ygate"))
    coef = torch.full((3, ycs), FILL, device=dev) if bn is not None else d["coef"].clone()
    dz, gv = d["dz"].clone(), GradView()
    gv.dz, gv.dpool, gv.coef = dz.data_ptr(), (d["dpool"].data_ptr() if "dpool" in d else None), coef.data_ptr()
    nrep, rs = pc._nrep(c), cout * cin + cout + 16
    gbuf = torch.zeros(nrep, rs, device=dev)
    dbp = C.c_void_p(gbuf.data_ptr() + 4 * cout * cin) if "dbias" in f else None
    dx, acc = (d["prior"].clone(), 1) if "prior" in d else (torch.full((n, h, w, xcs), pc.PREFILL, device=dev), 0)
    before = d["prior"] if "prior" in d else torch.full_like(dx, pc.PREFILL)
    o = pc.PwOpts()
    fs = _src(bn) if bn is not None else None
    args = [C.byref(vx), _lib.ptr(d["w"].contiguous()), C.byref(vy), C.byref(gv), _lib.ptr(dx), acc, _lib.ptr(gbuf), dbp, 1, None, nrep,
            C.c_int64(rs), C.byref(o), None, C.byref(fs) if fs is not None else None, None]
    L = _lib.lib()
    rc = L.lhn_conv_pw_bwd5(*args, _lib.stream()) if entry == 5 else L.lhn_conv_pw_bwd6(*args, flags, _lib.stream())
    torch.cuda.synchronize()
    _lib.check(rc, f"pw bwd{entry} {name}")
    tot = gbuf.sum(0)
    out = {"dw": tot[:cout * cin].view(cout, cin).cpu().numpy(), "dx": dx[..., xcoff:xcoff + cin].cpu().numpy(),
           "coef": coef.cpu().numpy(), "dz_after": dz.cpu().numpy(),
           "dw_pad_ok": np.array(bool((gbuf[:, cout * cin + (cout if dbp else 0):] == 0).all())),
           "dx_outside_ok": np.array(torch.equal(pc._outside(dx, xcoff, cin), pc._outside(before, xcoff, cin))),
           "dz_outside_ok": np.array(torch.equal(pc._outside(dz, ycoff, cout), pc._outside(d["dz"], ycoff, cout)))}
    if dbp:
        out["dbias"] = tot[cout * cin:cout * cin + cout].cpu().numpy()
    if bn is not None:
        out["dgamma"], out["dbeta"] = bn["dgamma"].cpu().numpy(), bn["dbeta"].cpu().numpy()
    return out


def _child(tmp, env_extra, names):
    out = os.path.join(str(tmp), "out.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out] + names, env=dict(os.environ, **env_extra),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return dict(np.load(out))


def _of(res, case, entry):
    pre = f"{case}/{entry}/"
    return {k[len(pre):]: v for k, v in res.items() if k.startswith(pre)}


@pytest.fixture(scope="module")
def split_runs(dev, tmp_path_factory):
    """Every case on the split path (which forms dy in place whatever the flag says), once per session."""
    return _child(tmp_path_factory.mktemp("pw_dzdead_split"), {"LHN_PW_BWD_SPLIT": "1"}, list(CASES))


@pytest.mark.parametrize("case", list(CASES))
def test_dz_dead_matches_float64_and_only_reads_dz(dev, split_runs, case):
    name = "dzdead_" + case
    c = pc._ALL["bwd"][name]
    xcs, xcoff, ycs, ycoff, ho, wo = pc.geometry("bwd", name)
    g = pc.inputs("bwd", name)
    bn = _bn(case)
    gref = g
    if bn is not None:                  # the coefficients of the separate launch: the reference's, and the fold's bit for bit
        sep, coef_sep = _on(bn, dev), torch.full((3, ycs), FILL, device=dev)
        _separate(sep, coef_sep, ycs, ycoff, c["cout"])
        gref = dict(g, coef=coef_sep.cpu())
    got = _run(case, dev, g, 6, DZ_DEAD, _on(bn, dev) if bn is not None else None)
    _same_bits(got["dz_after"], g["dz"].numpy(), f"{name}: dz was written")
    if bn is not None:
        _same_bits(got["coef"], coef_sep, f"{name} coef")
        _same_bits(got["dgamma"], sep["dgamma"], f"{name} dgamma")
        _same_bits(got["dbeta"], sep["dbeta"], f"{name} dbeta")
    r64 = pc.reference_bwd(name, gref)
    assert ("dbias" in r64) == ("dbias" in c["flags"]) and "dx" in r64 and "dz" not in r64
    old = _of(split_runs, case, 6)
    bad = []
    for k in OUTPUTS:
        if k not in r64:
            continue
        assert got[k].shape == r64[k].shape == old[k].shape, f"{name} {k}"
        e_new, e_old = pc.rel_err(got[k], r64[k]), pc.rel_err(old[k], r64[k])
        print(f"pw_bwd_dzdead {name} {k}: no dy store {e_new:.3e}  split {e_old:.3e}  bar {FACTOR * e_old:.3e}")
        if not e_new <= FACTOR * e_old:
            bad.append(f"{k}: {e_new:.3e} > {FACTOR} x {e_old:.3e}")
    bad += [f"{k}: floats outside the outputs changed" for k, v in got.items() if k.endswith("_ok") and not bool(v)]
    assert not bad, f"{name}: " + "; ".join(bad)


def test_dz_dead_equals_bwd5_bit_for_bit_in_deterministic_mode(dev, tmp_path):
    res = _child(tmp_path, {"LHN_DETERMINISTIC": "1"}, list(CASES))
    for case in CASES:
        a, b = _of(res, case, 5), _of(res, case, 6)
        assert set(a) == set(b) and "dx" in a and "dw" in a
        for k in a:
            if k == "dz_after":         # lhn_conv_pw_bwd5 leaves dy there, the flagged call the dz it was given
                assert not np.array_equal(a[k], b[k]), f"{case}: lhn_conv_pw_bwd5 did not store dy"
                _same_bits(b[k], pc.inputs("bwd", "dzdead_" + case)["dz"].numpy(), f"{case}: dz was written")
            else:
                _same_bits(a[k], b[k], f"{case} {k}")


# ---------------------------------------------------------------- the plan executor's flag, end to end
@pytest.mark.parametrize("model", ["block", "B"])
def test_train_step_is_bit_identical_with_and_without_the_dy_store(dev, tmp_path, model):
    res = []
    for store in ("1", "0"):
        out = str(tmp_path / f"store{store}.npz")
        r = subprocess.run([sys.executable, os.path.join(HERE, "pw_dzdead_child.py"), model, out],
                           env=dict(os.environ, LHN_PW_BWD_DY_STORE=store, LHN_DETERMINISTIC="1"), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        res.append(np.load(out))
    a, b = res
    assert set(a.files) == set(b.files) and any(k.startswith("g.") for k in a.files) and any(k.startswith("b.") for k in a.files)
    assert np.isfinite(a["loss"]) and float(np.abs(a["gflat"]).max()) > 0
    for k in a.files:
        _same_bits(a[k], b[k], k)


if __name__ == "__main__":
    dst, names = sys.argv[1], sys.argv[2:]
    device = torch.device("cuda:0")
    res = {}
    for nm in names:
        inp = pc.inputs("bwd", "dzdead_" + nm)
        for ent, fl in ((5, 0), (6, DZ_DEAD)):
            b_in = _bn(nm)
            for key, val in _run(nm, device, inp, ent, fl, _on(b_in, device) if b_in is not None else None).items():
                res[f"{nm}/{ent}/{key}"] = val
    np.savez(dst, **res)
