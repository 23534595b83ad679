"""The accumulating backward of the 32 -> 32 1x1 convolution: k_pw_bwd_wr with the prior dx in the tile prefetch (PF = 3, plain and
with reader-side BatchNorm sums; csrc/k_conv_pw.hip), called through lhn_conv_pw_bwd3 with dx_accumulate = 1 into a random prior.
Inputs, the kernel call and the references are those of tests/pw_cases.py; the cases below are added to its table in memory.
64 -> 64 keeps the read-modify-write at its store and has no case here.

Pixel counts against the 128-pixel tile: 9 = under one tile; 200 = one tile and a tail; 384 = whole tiles only; 640 = five tiles,
more than the four workgroups of deterministic mode.  Each with: acc | acc bns | acc dbias at one gradient replica | acc views
(x / dx at channel 64, y / dz at channel 32 of wider buffers) | acc xgate.

(a) every element of dx, dW, dbias and both sums against float64 at the bar of tests/test_pw_gpu.py: max(2e-5, 3 x the error of the
    same reference computed in float32 on the CPU);
(b) the accumulate is ONE fp32 add: the same inputs run with dx_accumulate = 0 into a prefilled dx give dX, and the accumulating call's
    dx must be float32(prior + dX) bit for bit;
(c) dz keeps its bits, every float outside the views keeps its bits, sum replicas that no workgroup owns stay zero;
(d) LHN_PW_BWD_ACC_PREFETCH=0 (a child process: the read-modify-write of the PF = 2 instances) gives the same bits of dx in every
    mode, and under LHN_DETERMINISTIC=1 in both processes the same bits of dW, dbias and the sums as well.

Measured (profiles/parity_pw_bwd_acc.json, 20 cases): largest error against float64 1.8e-7 for dx, 1.5e-7 for dW, 1.7e-7 for dbias,
2.7e-7 for the sums, all at the 2e-5 floor of the bar; no element of dx off float32(prior + dX) in any case.

Run as a script it is the child: python tests/test_pw_bwd_acc_gpu.py OUT.npz NAME ..."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import pw_cases as pc
from conftest import parity_record

pytestmark = pytest.mark.gpu
PIXELS = {"tiny": (1, 3, 3), "tail": (2, 10, 10), "tiles": (6, 8, 8), "loop": (10, 8, 8)}
FLAGS = {"acc": ("acc", {}), "bns": ("acc bns", {}), "dbias": ("acc dbias", {"nrep": 1}), "views": ("acc views", {}),
         "xgate": ("acc xgate", {})}
CASES, STORE = {}, {}
for _tag, _nhw in PIXELS.items():
    for _nm, (_fl, _kw) in FLAGS.items():
        CASES[f"accpf_32_32_{_nm}_{_tag}"] = pc._case(32, 32, _nhw, _fl, **_kw)
        STORE[f"accpf_32_32_{_nm}_{_tag}_store"] = pc._case(32, 32, _nhw, _fl.replace("acc", "").strip(), **_kw)      # (b): the same call, stored
pc._ALL["bwd"].update(CASES)
pc._ALL["bwd"].update(STORE)
OUTPUTS = ("dx", "dw", "dbias", "sums_du", "sums_duxhat")

_REF = {}


def _reference(name):
    """Inputs, the float64 reference and the bar per output; computed once per session."""
    import torch
    if name not in _REF:
        g = pc.inputs("bwd", name)
        r64, r32 = pc.reference_bwd(name, g), pc.reference_bwd(name, g, torch.float32)
        _REF[name] = (g, r64, {k: max(2e-5, 3 * pc.rel_err(r32[k], r64[k])) for k in r64})
    return _REF[name]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _child(tmp, env_extra, names):
    out = os.path.join(str(tmp), "out.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out] + names, env=dict(os.environ, **env_extra),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return dict(np.load(out))


def _of(res, name):
    pre = f"{name}/"
    return {k[len(pre):]: v for k, v in res.items() if k.startswith(pre)}


@pytest.fixture(scope="module")
def children(dev, tmp_path_factory):
    """Every case in three child processes: the switch at 0, deterministic mode, and both."""
    runs = {}
    for tag, env in (("rmw", {"LHN_PW_BWD_ACC_PREFETCH": "0"}), ("det", {"LHN_DETERMINISTIC": "1", "LHN_PW_BWD_ACC_PREFETCH": "1"}),
                     ("det_rmw", {"LHN_DETERMINISTIC": "1", "LHN_PW_BWD_ACC_PREFETCH": "0"})):
        runs[tag] = _child(tmp_path_factory.mktemp("pw_bwd_acc_" + tag), env, list(CASES))
    return runs


@pytest.mark.parametrize("name", list(CASES))
def test_pw_bwd_acc_matches_float64_and_adds_once(dev, name):
    g, r64, bar = _reference(name)
    got = pc.run_bwd(name, dev, g)
    c = CASES[name]
    assert set(r64) <= set(got) and ("dbias" in got) == ("dbias" in c["flags"]) and ("sums_du" in got) == ("bns" in c["flags"])
    bad = []
    for k in OUTPUTS:                                                        # (a)
        if k not in r64:
            continue
        assert got[k].shape == r64[k].shape, f"{name} {k}: shapes {got[k].shape} {r64[k].shape}"
        e = pc.rel_err(got[k], r64[k])
        e = e if np.isfinite(e) else float("inf")
        parity_record(f"pw_bwd_acc/{name}", **{f"{k}_err": e, f"{k}_bar": bar[k]})
        print(f"pw_bwd_acc {name} {k}: {e:.3e}  bar {bar[k]:.3e}")
        if not e <= bar[k]:
            bad.append(f"{k}: {e:.3e} > {bar[k]:.3e}")
    for k, v in got.items():                                                 # (c)
        if k.endswith("_ok") and not bool(v):
            bad.append(f"{k}: floats that must keep their bits changed")
    assert "dz_outside_ok" in got and "dx_outside_ok" in got and "dz" not in got
    # (b) the same inputs without the prior: dx_accumulate = 0 into the prefill
    xcoff = pc.geometry("bwd", name)[1]
    stored = pc.run_bwd(name + "_store", dev, {k: v for k, v in g.items() if k != "prior"})
    want = g["prior"][..., xcoff:xcoff + c["cin"]].numpy() + stored["dx"]
    assert want.dtype == np.float32
    ndiff = int((_bits(got["dx"]) != _bits(want)).sum())
    parity_record(f"pw_bwd_acc/{name}", dx_bits_off_prior_plus_store=ndiff)
    if ndiff:
        bad.append(f"dx differs from float32(prior + stored dX) in {ndiff} of {want.size} elements")
    assert not bad, f"{name}: " + "; ".join(bad)


def _sum_replicas(name, dev, g):
    """The accumulating call of pc.run_bwd for a sums case, returning the 32 replicas of the sums un-added."""
    import torch
    c = CASES[name]
    cin, cout = c["cin"], c["cout"]
    d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in g.items()}
    vx = pc._view(d["x"], 0, cin, d["xtab"])
    vy = pc._view(d["y"], 0, cout, d["ytab"])
    dz = d["dz"].clone()
    gv = pc.GradView()
    gv.dz, gv.dpool, gv.coef = dz.data_ptr(), None, d["coef"].data_ptr()
    nrep, rs = pc._nrep(c), cout * cin + cout + 16
    gbuf = torch.zeros(nrep, rs, device=dev)
    dx = d["prior"].clone()
    sums = torch.zeros(32, 2, 128, dtype=torch.float64, device=dev)
    bs = pc.BnSum()
    bs.sums, bs.save, bs.C, bs.coff = sums.data_ptr(), d["save"].data_ptr(), 128, 64
    o = pc.PwOpts()
    wdev = d["w"].contiguous()
    rc = pc._lib.lib().lhn_conv_pw_bwd3(C.byref(vx), pc._lib.ptr(wdev), C.byref(vy), C.byref(gv), pc._lib.ptr(dx), 1, pc._lib.ptr(gbuf), None, 1,
                                        None, nrep, C.c_int64(rs), C.byref(o), C.byref(bs), pc._lib.stream())
    torch.cuda.synchronize()
    pc._lib.check(rc, f"pw bwd {name}")
    return sums.cpu().numpy()


@pytest.mark.parametrize("name", [n for n in CASES if "bns" in CASES[n]["flags"]])
def test_pw_bwd_acc_sum_replicas(dev, name):
    """(c) workgroup b adds into replica b % 32 and into no other: one workgroup per tile, four at the most under LHN_DETERMINISTIC=1."""
    g, r64, bar = _reference(name)
    c = CASES[name]
    ntiles = (c["nhw"][0] * c["nhw"][1] * c["nhw"][2] + 127) // 128
    wgs = min(ntiles, 4) if os.environ.get("LHN_DETERMINISTIC") == "1" else ntiles
    assert wgs < 32
    sums = _sum_replicas(name, dev, g)
    assert not sums[wgs:].any(), f"{name}: replicas beyond the {wgs} workgroups were written"
    assert all(sums[r, :, 64:96].any() for r in range(wgs)), f"{name}: a workgroup's replica is empty"
    tot = sums.sum(0)[:, 64:96]
    for i, k in enumerate(("sums_du", "sums_duxhat")):
        assert pc.rel_err(tot[i], r64[k]) <= bar[k], f"{name} {k}"


@pytest.mark.parametrize("name", list(CASES))
def test_pw_bwd_acc_switch_keeps_the_bits(dev, children, name):
    """(d) the read-modify-write of LHN_PW_BWD_ACC_PREFETCH=0 against the prefetched prior."""
    g, r64, bar = _reference(name)
    here = pc.run_bwd(name, dev, g)
    rmw, det, det_rmw = (_of(children[t], name) for t in ("rmw", "det", "det_rmw"))
    assert set(here) == set(rmw) == set(det) == set(det_rmw) and "dx" in here
    for tag, other in (("default", rmw), ("deterministic, prefetch", det), ("deterministic, read-modify-write", det_rmw)):
        np.testing.assert_array_equal(_bits(here["dx"]), _bits(other["dx"]), err_msg=f"{name}: dx of this process against {tag}")
        assert all(bool(v) for k, v in other.items() if k.endswith("_ok")), f"{name} ({tag})"
    for k in det:
        if not k.endswith("_ok"):
            np.testing.assert_array_equal(det[k].view(np.uint32), det_rmw[k].view(np.uint32), err_msg=f"{name} {k}: deterministic mode, switch 1 against 0")
    for k in OUTPUTS:        # the switched-off path still answers
        if k in r64:
            assert pc.rel_err(rmw[k], r64[k]) <= bar[k] and pc.rel_err(det_rmw[k], r64[k]) <= bar[k], f"LHN_PW_BWD_ACC_PREFETCH=0 {name} {k}"


if __name__ == "__main__":
    import torch
    dst, names = sys.argv[1], sys.argv[2:]
    device = torch.device("cuda:0")
    res = {}
    for nm in names:
        for key, val in pc.run_bwd(nm, device, pc.inputs("bwd", nm)).items():
            res[f"{nm}/{key}"] = val
    np.savez(dst, **res)
