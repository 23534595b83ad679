"""The register-W backward of the narrow 1x1 convolutions (k_pw_bwd_wr: 64 -> 64 at 64-pixel tiles, 32 -> 32 at 128-pixel tiles,
each plain and with reader-side BatchNorm sums), called through lhn_conv_pw_bwd3 and compared element by element (dx, dW, dbias,
the BatchNorm sums) with a float64 computation on the CPU.  Inputs, the kernel call and the reference are those of
tests/pw_cases.py; the cases below are added to its table in memory.

Bar: k_pw_bwd (the code before these instances, reached with LHN_PW_BWD_NARROW=0 in a child process) runs the same cases in the
same session; for each output the new kernel's largest error against float64, relative to the output's largest magnitude, may
be at most twice k_pw_bwd's: another fp32 summation order over the same terms.

dz: the fused path only reads dz, so in every case dz must keep its bits (the `dz_outside_ok` flag of pc.run_bwd compares the
whole buffer), as must every float outside the views.  A sums case must leave every replica no workgroup owns at zero.

Summation orders: with one tile per workgroup 64 -> 64 adds the same terms in the same order as k_pw_bwd<64,2> (same tile, same
wave roles, same K order), so equal bits on the two paths are expected there and say nothing about the switch.  They part where
the grids part: under LHN_DETERMINISTIC=1 the new kernel runs four workgroups and k_pw_bwd six, so at five tiles tile 4 joins
tile 0 in the accumulators of one workgroup where k_pw_bwd gives each tile a replica of its own, and the bits of dW differ
(asserted in test_pw_bwd_narrow_deterministic).  32 -> 32 sums dW over four 32-pixel quarters of a 128-pixel tile where
k_pw_bwd<32,1> takes two halves of a 64-pixel tile: from 128 pixels on its bits differ in every mode.

Measured (profiles/parity_pw_bwd_narrow.json, 48 entries, 149 outputs): errors of 5e-8 .. 4e-7 on both paths; 118 outputs have the
same error as k_pw_bwd (every dx; 64 -> 64 throughout outside deterministic mode); the largest ratio new / old is 1.75 (dbias of
32 -> 32 at 200 pixels: 1.69e-7 against 9.64e-8), the largest for dW 1.59 (same case).

Run as a script it is the child: python tests/test_pw_bwd_narrow_gpu.py OUT.npz REPEATS NAME ..."""
import ctypes as C
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
PAIRS = ((64, 64), (32, 32))
TILE = {64: 64, 32: 128}          # pixels per tile of the instance that takes Cin = Cout = key
# pixel counts against the 64-pixel tile: 9 = under one tile; 70 = one tile and a 6-row tail; 192 = whole tiles only; 320 = five
# tiles, more than the four workgroups of deterministic mode
PIXELS = {"tiny": (1, 3, 3), "tail": (2, 5, 7), "tiles": (3, 8, 8), "loop": (5, 8, 8)}
# the same situations against the 128-pixel tile of 32 -> 32 (tiny and tail already sit under one such tile):
# 200 = one tile and a tail; 384 = three whole tiles; 640 = five tiles
PIXELS128 = {"tail128": (2, 10, 10), "tiles128": (6, 8, 8), "loop128": (10, 8, 8)}

CASES = {}
for _c, _ in PAIRS:
    _sizes = dict(PIXELS, **(PIXELS128 if TILE[_c] == 128 else {}))
    for _tag, _nhw in _sizes.items():
        CASES[f"narrow_{_c}_{_c}_{_tag}"] = pc._case(_c, _c, _nhw, "dbias")
        CASES[f"narrow_{_c}_{_c}_bns_{_tag}"] = pc._case(_c, _c, _nhw, "bns")       # reader-side sums
    # variations at 70 pixels (always: pending table with leaky slope 0.1 on x and y, non-trivial A | B | C, dx prefilled)
    for _nm, _fl, _kw in (("store", "", {}),                             # dx_accumulate = 0 into a dx that holds 7.0
                          ("acc", "acc", {}),                            # dx_accumulate = 1 into a random prior
                          ("nodx", "nodx", {}),                          # dx = NULL
                          ("nrep1", "dbias acc", {"nrep": 1}),           # one gradient replica (the base cases: four)
                          ("xgate", "xgate", {}),
                          ("views", "views dbias", {}),                  # x / dx at channel 64, y / dz at channel 32 of wider buffers
                          ("ygate_dpool", "ygate dpool", {})):           # the terms of lhn_grad_du that need pixel coordinates
        CASES[f"narrow_{_c}_{_c}_{_nm}"] = pc._case(_c, _c, PIXELS["tail"], _fl, **_kw)
pc._ALL["bwd"].update(CASES)          # (not pc.BWD: tests/test_pw_gpu.py parametrises over that)
DET_CASES = [n for n in CASES if n.endswith(("_tiles", "_loop", "_tiles128", "_loop128"))]
BNS_CASES = [n for n in CASES if "bns" in CASES[n]["flags"]]
OUTPUTS = ("dx", "dw", "dbias", "sums_du", "sums_duxhat")

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
def old_runs(dev, tmp_path_factory):
    """Every case on k_pw_bwd, once per session."""
    return _child(tmp_path_factory.mktemp("pw_bwd_old"), {"LHN_PW_BWD_NARROW": "0"}, list(CASES), 1)


def _compare(name, got, old, tag=""):
    """Every output of the float64 reference, every element: new error <= FACTOR x k_pw_bwd's error on the same case."""
    _, r64 = _reference(name)
    bad = []
    for k in OUTPUTS:
        if k not in r64:      # (dx = NULL, no dbias, no sums)
            continue
        assert got[k].shape == r64[k].shape == old[k].shape, f"{name} {k}: shapes {got[k].shape} {old[k].shape} {r64[k].shape}"
        e_new, e_old = pc.rel_err(got[k], r64[k]), pc.rel_err(old[k], r64[k])
        if not np.isfinite(e_new):
            e_new = float("inf")
        parity_record(f"pw_bwd_narrow/{tag}{name}", **{f"{k}_err_wr": e_new, f"{k}_err_old": e_old, f"{k}_bar": FACTOR * e_old})
        print(f"pw_bwd_narrow {tag}{name} {k}: k_pw_bwd_wr {e_new:.3e}  k_pw_bwd {e_old:.3e}  bar {FACTOR * e_old:.3e}")
        if not e_new <= FACTOR * e_old:
            bad.append(f"{k}: {e_new:.3e} > {FACTOR} x {e_old:.3e}")
    for k, v in got.items():
        if k.endswith("_ok") and not bool(v):
            bad.append(f"{k}: floats that must keep their bits changed")
    assert not bad, f"{tag}{name}: " + "; ".join(bad)


@pytest.mark.parametrize("name", list(CASES))
def test_pw_bwd_narrow_matches_float64(dev, old_runs, name):
    g, r64 = _reference(name)
    got = pc.run_bwd(name, dev, g)
    c = CASES[name]
    assert ("dx" in got) == ("nodx" not in c["flags"]) and ("dbias" in got) == ("dbias" in c["flags"])
    assert ("sums_du" in got) == ("bns" in c["flags"]) and "dz_outside_ok" in got and "dz" not in got
    _compare(name, got, _of(old_runs, name, 0))


def _sum_replicas(name, dev, g):
    """The call of pc.run_bwd for a sums case, returning the 32 replicas of the sums un-added."""
    import torch
    c = CASES[name]
    (n, h, w), cin, cout = c["nhw"], c["cin"], c["cout"]
    d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in g.items()}
    vx = pc._view(d["x"], 0, cin, d["xtab"])
    vy = pc._view(d["y"], 0, cout, d["ytab"])
    dz = d["dz"].clone()
    gv = pc.GradView()
    gv.dz, gv.dpool, gv.coef = dz.data_ptr(), None, d["coef"].data_ptr()
    nrep, rs = pc._nrep(c), cout * cin + cout + 16
    gbuf = torch.zeros(nrep, rs, device=dev)
    dx = torch.full((n, h, w, cin), pc.PREFILL, device=dev)
    sums = torch.zeros(32, 2, 128, dtype=torch.float64, device=dev)
    bs = pc.BnSum()
    bs.sums, bs.save, bs.C, bs.coff = sums.data_ptr(), d["save"].data_ptr(), 128, 64
    o = pc.PwOpts()
    wdev = d["w"].contiguous()
    rc = pc._lib.lib().lhn_conv_pw_bwd3(C.byref(vx), pc._lib.ptr(wdev), C.byref(vy), C.byref(gv), pc._lib.ptr(dx), 0, pc._lib.ptr(gbuf), None, 1,
                                        None, nrep, C.c_int64(rs), C.byref(o), C.byref(bs), pc._lib.stream())
    torch.cuda.synchronize()
    pc._lib.check(rc, f"pw bwd {name}")
    return sums.cpu().numpy()


@pytest.mark.parametrize("name", BNS_CASES)
def test_pw_bwd_narrow_sum_replicas(dev, name):
    """Workgroup b adds into replica b % 32 and into no other: with fewer workgroups than replicas the rest stays exactly zero
    (one workgroup per tile; four at the most under LHN_DETERMINISTIC=1)."""
    g, r64 = _reference(name)
    c = CASES[name]
    m = c["nhw"][0] * c["nhw"][1] * c["nhw"][2]
    ntiles = (m + TILE[c["cin"]] - 1) // TILE[c["cin"]]
    wgs = min(ntiles, 4) if os.environ.get("LHN_DETERMINISTIC") == "1" else ntiles
    assert wgs < 32
    sums = _sum_replicas(name, dev, g)
    assert not sums[wgs:].any(), f"{name}: replicas beyond the {wgs} workgroups were written"
    assert all(sums[r, :, 64:64 + c["cin"]].any() for r in range(wgs)), f"{name}: a workgroup's replica is empty"
    tot = sums.sum(0)[:, 64:64 + c["cin"]]
    for i, k in enumerate(("sums_du", "sums_duxhat")):      # (that this call is the one pc.run_bwd makes: the floor of tests/test_pw_gpu.py's bar)
        assert pc.rel_err(tot[i], r64[k]) <= 2e-5, f"{name} {k}"


def test_pw_bwd_narrow_deterministic(dev, tmp_path):
    """LHN_DETERMINISTIC=1: four workgroups, so a workgroup walks more than one tile; two runs agree bit for bit and meet the
    bar against k_pw_bwd under the same switch.  The switch is visible here for 64 -> 64: at 320 pixels workgroup 0 of the new
    kernel continues its dW accumulators from tile 0 into tile 4, while k_pw_bwd (six workgroups) sums the two tiles apart
    and they meet in the sum over the replicas: another association in each of the 4,096 elements, so the bits of dW differ."""
    new = _child(tmp_path, {"LHN_DETERMINISTIC": "1"}, DET_CASES, 2)
    old_dir = tmp_path / "old"
    old_dir.mkdir()
    old = _child(old_dir, {"LHN_DETERMINISTIC": "1", "LHN_PW_BWD_NARROW": "0"}, DET_CASES, 1)
    for name in DET_CASES:
        a, b = _of(new, name, 0), _of(new, name, 1)
        assert a and set(a) == set(b), name
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{name} {k}")
        _compare(name, a, _of(old, name, 0), "deterministic/")
    for name in ("narrow_64_64_loop", "narrow_64_64_bns_loop"):
        assert not np.array_equal(_of(new, name, 0)["dw"], _of(old, name, 0)["dw"]), f"{name}: the switch did not change the kernel"


def test_pw_bwd_narrow_switch_takes_the_old_path(dev, old_runs):
    """LHN_PW_BWD_NARROW=0: k_pw_bwd still answers (the float64 bar of tests/test_pw_gpu.py), and for 32 -> 32 it is visibly another
    kernel than the default.  At 192 pixels the default adds the first 128 as ((q0 + q1) + q2) + q3, four waves' quarters met in
    LDS, where k_pw_bwd adds (q0 + q1) and (q2 + q3) in two workgroups' replicas: another association of the same four terms in
    each of the 1,024 elements, so the bits of dW differ.  (At 70 pixels both paths form (q0 + q1) + q2: equal bits are possible
    there.)  64 -> 64 with one tile per workgroup adds the same terms in the same order on both paths; its case is the five-tile
    one under LHN_DETERMINISTIC=1, asserted in test_pw_bwd_narrow_deterministic on the children that test runs."""
    import torch
    for name in ("narrow_64_64_tail", "narrow_32_32_tail", "narrow_32_32_tiles", "narrow_64_64_bns_tail", "narrow_32_32_bns_tail"):
        g, r64 = _reference(name)
        r32 = pc.reference_bwd(name, g, torch.float32)
        old = _of(old_runs, name, 0)
        for k, ref in r64.items():
            bar = max(2e-5, 3 * pc.rel_err(r32[k], ref))
            assert pc.rel_err(old[k], ref) <= bar, f"LHN_PW_BWD_NARROW=0 {name} {k}"
        assert all(bool(v) for k, v in old.items() if k.endswith("_ok")), name
        if name == "narrow_32_32_tiles":
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
