"""The dense 3x3 convolution at 40 and 160 channels (mynet at width 160) through the C ABI, per element against float64
(tests/kxk160_cases.py lists the cases, profiles/kxk160_instances.md which kernel instance each reaches): K = 160 as five 32-channel
slices per tap, 160 features as five tiles in a block or over gridDim.y = 5, the weight gradient over a 128- and a 32-channel input
slice; K = 40 on the 64-channel images with a zero tail, dy on the fly by default and plain under LHN_PLAIN=1 or a pooled gradient.
Bar as in tests/test_kxk_gpu.py: max(2e-5, 3 * e32) with e32 the error of torch's float32 CPU run of the same case, every `*_ok`
guard of the harness (slack behind dW replicas and the scratch, floats outside views, dz).  Every case but the refusals stops with
"unsupported channels" on a library without these instances."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kxk160_cases as k6
import kxk_cases as kc
from conftest import parity_record

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FLOOR = 2e-5

_REF = {}


def _reference(kind, name):
    key = (kind, name)
    if key in _REF:
        return _REF[key]
    g = kc.inputs(kind, name)
    r64, r32 = kc.reference(kind, name, g), kc.reference(kind, name, g, torch.float32)
    e32 = {k: kc.rel_err(r32[k], r64[k]) for k in r64}
    if not name.startswith("big_"):      # (193 x 193 x 160: 24 MB per tensor, used by one test each)
        _REF[key] = (g, r64, e32)
    return g, r64, e32


def _check(kind, name, got, r64, e32, tag):
    """Every output of the reference that the call produced, every element; every `*_ok` flag.  `dz` is an output on the plain path only
    (the harness leaves it out elsewhere and reports `dz_unchanged_ok` instead)."""
    bad = []
    for k, ref in r64.items():
        if k == "dz" and "dz" not in got:
            assert "dz_unchanged_ok" in got, f"{kind}:{name}: neither dz nor dz_unchanged_ok"
            continue
        assert got[k].shape == ref.shape, f"{kind}:{name} {k}: shape {got[k].shape} vs {ref.shape}"
        err, bar = kc.rel_err(got[k], ref), max(FLOOR, 3 * e32[k])
        if not np.isfinite(err):
            err = float("inf")
        parity_record(f"kxk160/{tag}{kind}_{name}", **{f"{k}_err": err, f"{k}_e32": e32[k], f"{k}_bar": bar})
        print(f"kxk160 {tag}{kind}:{name} {k}: err {err:.3e} e32 {e32[k]:.3e} bar {bar:.3e}")
        if not err <= bar:
            bad.append(f"{k}: err {err:.3e} > bar {bar:.3e}")
    flags = [k for k in got if k.endswith("_ok")]
    assert flags, f"{kind}:{name}: no sentinel flags"
    for k in flags:
        if not bool(got[k]):
            bad.append(f"{k}: floats that must keep their bits changed")
    assert not bad, f"{tag}{kind}:{name}: " + "; ".join(bad)


def _child(tmp_path, env_extra, names, reps, timeout):
    out = str(tmp_path / "out.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("LHN_PLAIN", "LHN_DETERMINISTIC")}
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.join(HERE, "kxk160_cases.py"), out, str(reps)] + names, env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return dict(np.load(out))


def _of(res, full, rep):
    pre = f"{full}/{rep}/"
    return {k[len(pre):]: v for k, v in res.items() if k.startswith(pre)}


@pytest.mark.parametrize("name", list(k6.FWD))
def test_kxk160_fwd_matches_float64(dev, name):
    g, r64, e32 = _reference("fwd", name)
    _check("fwd", name, kc.run_fwd(name, dev, g), r64, e32, "")


@pytest.mark.parametrize("name", list(k6.BWD))
def test_kxk160_bwd_matches_float64(dev, name):
    c = k6.BWD[name]
    assert kc.plain_path(c) == (c["cin"] == 160 or "dpool" in c["flags"])
    g, r64, e32 = _reference("bwd", name)
    got = kc.run_bwd(name, dev, g)
    assert ("dz" in got) == kc.plain_path(c)
    _check("bwd", name, got, r64, e32, "")


def test_kxk160_fwd_stem_concat(dev):
    """40 -> 40 stride 2 into channels [0, 40) of an 80-wide buffer (my_pelee_stem's concatenation): the other half keeps its bits."""
    g, r64, e32 = _reference("fwd", k6.CONCAT_CASE)
    _check("fwd", k6.CONCAT_CASE, k6.run_fwd_concat(dev, g), r64, e32, "concat/")


@pytest.mark.parametrize("c", k6.WIDTHS)
def test_kxk160_bwd_stride2_lattice(dev, c):
    """One tap of W at a time (tests/test_kxk_gpu.py::test_kxk_bwd_stride2_lattice): tap (kh, kw) reaches only the input pixels of its
    parity class, every other pixel is stored as an exact zero, and the class meets the float64 bar."""
    name = f"s2_{c}_{c}_odd_store"
    g, _, _ = _reference("bwd", name)
    for tap in range(9):
        kh, kw = divmod(tap, 3)
        g1 = dict(g)
        g1["w"] = torch.zeros_like(g["w"])
        g1["w"][:, :, kh, kw] = g["w"][:, :, kh, kw]
        r64, r32 = kc.reference_bwd(name, g1), kc.reference_bwd(name, g1, torch.float32)
        got = kc.run_bwd(name, dev, g1)
        _check("bwd", name, got, r64, {k: kc.rel_err(r32[k], r64[k]) for k in r64}, f"tap{tap}/")
        reached = np.zeros(got["dx"].shape[1:3], bool)
        reached[(kh + 1) % 2::2, (kw + 1) % 2::2] = True
        assert not got["dx"][:, ~reached].any(), f"{name} tap {tap}: a pixel outside the tap's parity class received a gradient"
        assert got["dx"][:, reached].any()


def test_kxk160_fwd_fused_finalize(dev):
    """fin != NULL with gridDim.y = 5: the last of gridDim.x * gridDim.y workgroups folds the statistics -- table, mean | invstd and
    running statistics against float64, the table outside the slice untouched, one ticket per workgroup."""
    g = k6.fin_inputs()
    r64, r32 = k6.reference_fwd_fin(g), k6.reference_fwd_fin(g, torch.float32)
    got = k6.run_fwd_fin(dev, g)
    assert int(got["grid_y"]) == 5 and bool(got["tickets_ok"]), got["tickets"]      # 3 tiles x 5: exactly 15 tickets
    assert int(got["fin_nbt"][0]) == 6
    _check("fwd", "fin_160_160", {k: v for k, v in got.items() if k in r64 or k.endswith("_ok")}, r64,
           {k: kc.rel_err(r32[k], r64[k]) for k in r64}, "")


WT_CASES = [f"fwd:{n}" for n in k6.FWD if not n.startswith("big_")] + [f"bwd:{n}" for n in k6.BWD if n.startswith(("pair_", "s2_"))]


@pytest.mark.parametrize("full", WT_CASES)
def test_kxk160_wt_scratch_bits(dev, full):
    """wt_scratch = NULL (weights gathered from w[co][ci][tap], slice by slice, the zero tail of K = 40 by the same guard) against the
    tap-major copy: the same products in the same order, so y and dx agree bit for bit."""
    kind, name = full.split(":")
    g, r64, e32 = _reference(kind, name)
    run = kc.run_fwd if kind == "fwd" else kc.run_bwd
    a, b = run(name, dev, g, wt=True), run(name, dev, g, wt=False)
    out = "y" if kind == "fwd" else "dx"
    np.testing.assert_array_equal(a[out], b[out], err_msg=full)
    _check(kind, name, b, r64, e32, "nowt/")
    assert bool(a["wt_ok"]) and "wt_ok" not in b


MT_CASES = [f"fwd:{n}" for n in k6.FWD if n.startswith("mt_")] + [f"bwd:{n}" for n in k6.BWD if n.startswith("mt_")]
BWD40 = [f"bwd:{n}" for n, c in k6.BWD.items() if c["cin"] == 40]
BWD160 = [f"bwd:{n}" for n, c in k6.BWD.items() if c["cin"] == 160 and not n.startswith("big_")]


def test_kxk160_deterministic_bits(dev, tmp_path):
    """LHN_DETERMINISTIC=1: grids sized for 2 CUs, so every 160 case from 4 tiles on runs k_kxk<160, 5, ...> -- five feature tiles in one
    block, the instance of the workload's large maps -- in a persistent loop with the next tile's first slice in flight: with views and
    gates (view_160_160), a pooled gradient and views (full_160_160), stride 2 forward and by parity class (s2mt_160_160), and the
    15-tile cases; dW in 16 exclusive replicas; two runs agree bit for bit.  Every 40-channel backward case runs too."""
    names = list(k6.DET)
    for full in names:
        kind, name = full.split(":")
        if "_160_160" in name:
            assert "k_kxk<160, 5, " in kc.kernel_of(kind, name, cus=2), full
    res = _child(tmp_path, {"LHN_DETERMINISTIC": "1"}, names + [f"fwd:fin@{k6.FIN_DET}"], 2, timeout=180)
    fin = _of(res, f"fwd:fin@{k6.FIN_DET}", 0)           # the fused finalize with gridDim.y = 1 (NT = 5)
    assert int(fin["grid_y"]) == 1 and bool(fin["tickets_ok"]), fin["tickets"]
    f64, f32 = k6.reference_fwd_fin(case=k6.FIN_DET), k6.reference_fwd_fin(dtype=torch.float32, case=k6.FIN_DET)
    _check("fwd", f"fin_{k6.FIN_DET}", {k: v for k, v in fin.items() if k in f64 or k.endswith("_ok")}, f64,
           {k: kc.rel_err(f32[k], f64[k]) for k in f64}, "deterministic/")
    for full in names:
        kind, name = full.split(":")
        _, r64, e32 = _reference(kind, name)
        a, b = _of(res, full, 0), _of(res, full, 1)
        assert a and a.keys() == b.keys()
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{full} {k}")
        _check(kind, name, a, r64, e32, "deterministic/")


@pytest.mark.parametrize("plain", ["0", "1"])
def test_kxk160_plain_switch(dev, tmp_path, plain):
    """LHN_PLAIN=0 / 1: every 40-channel backward case follows the switch (a pooled gradient stays plain under 0), every 160-channel
    case is plain under both -- the harness's plain_path, evaluated in the child, decides whether dz is an output -- and all meet
    the float64 bar."""
    names = BWD40 + BWD160
    res = _child(tmp_path, {"LHN_PLAIN": plain}, names, 1, timeout=180)
    for full in names:
        kind, name = full.split(":")
        c = k6.BWD[name]
        g, r64, e32 = _reference(kind, name)
        got = _of(res, full, 0)
        want_plain = c["cin"] == 160 or "dpool" in c["flags"] or plain == "1"
        assert ("dz" in got) == want_plain and ("dz_unchanged_ok" in got) != want_plain, f"{full}: path under LHN_PLAIN={plain}"
        _check(kind, name, got, r64, e32, f"LHN_PLAIN={plain}/")


@pytest.mark.parametrize("name", list(k6.FWD_REFUSE))
def test_kxk160_fwd_refuses(dev, name):
    rc, kept = kc.run_fwd(name, dev, expect_fail=True)
    assert rc != 0 and k6.FWD_REFUSE[name]["refuse"] in kc._lib.lib().lhn_last_error().decode()
    assert all(kept.values()), f"{name}: a refused call wrote to {[k for k, v in kept.items() if not v]}"


@pytest.mark.parametrize("name", list(k6.BWD_REFUSE))
def test_kxk160_bwd_refuses(dev, name):
    rc, kept = kc.run_bwd(name, dev, expect_fail=True)
    assert rc != 0 and k6.BWD_REFUSE[name]["refuse"] in kc._lib.lib().lhn_last_error().decode()
    assert all(kept.values()), f"{name}: a refused call wrote to {[k for k, v in kept.items() if not v]}"
