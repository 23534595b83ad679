"""The BatchNorm-backward finalize on the consumer side (include/lhn.h: lhn_bnbwdsrc, lhn_conv_dw_bwd4, lhn_conv_pw_bwd4) against
the separate launch, through the C ABI.  Every case runs both paths on the same inputs and the same sums buffer:

    old: lhn_bn_bwd_finalize2, then the existing backward entry (tests/dw_bwd_cases.py: run, tests/pw_cases.py: run_bwd);
    new: the new entry with the finalize source (k_dw3_bwd_rows / k_pw_bwd_wr fold the replicas in their prologue; every other
         kernel gets the finalize launch from the launcher).

coef (the whole table, the floats outside the BatchNorm's slice included), dgamma, dbeta and dx must agree bit for bit -- the fold
keeps the replica order and the double arithmetic of k_bn_bwd_finalize, and dx has one writer per element.  dW, the dy stored over
dz by the wide 1x1 kernels, dbias and the reader-side sums go through float atomics or are checked anyway: they meet the per-element
float64 bars of tests/test_dw_bwd_gpu.py / tests/test_pw_gpu.py, max(2e-5, 3 x the float32 error of the reference), with the
reference taken on the coefficients the separate launch wrote.  Shapes: the smallest that reach every branch, N = 2.

End to end: one train step of variant B (64 x 64 input, batch 2, LHN_DETERMINISTIC=1) in two fresh processes, LHN_BWD_FIN_CONSUMER=0
and =1 (read once per process): loss, every gradient and every running statistic bit-identical."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dw_bwd_cases as dc
import pw_cases as pc
from litehandnet_amd import _lib
from litehandnet_amd._lib import GradView

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 2e-5
FILL = 7.0          # coefficient floats outside the BatchNorm's slice


class BnBwdSrc(C.Structure):     # lhn_bnbwdsrc (include/lhn.h)
    _fields_ = [("sums", C.c_void_p), ("save", C.c_void_p), ("gamma", C.c_void_p), ("dgamma", C.c_void_p), ("dbeta", C.c_void_p),
                ("count", C.c_double), ("pgrad_scale", C.c_float), ("stat_channels", C.c_int32)]


# ---------------------------------------------------------------- cases (registered with the helpers' tables, which stay as they are)
# name: (helper case, BatchNorm extras): sc = channel stride of sums / save, prior = dgamma / dbeta hold values on entry,
# pscale = pgrad_scale, nogamma = gamma NULL
DW = {
    "c32_16": (dc._case(2, 16, 16, 32, 0, 32, 1, ""), {}),
    "c64_9x37": (dc._case(2, 9, 37, 64, 0, 64, 1, ""), {}),                         # two lead blocks, row and column tails
    "c40_8": (dc._case(2, 8, 8, 40, 0, 40, 1, ""), {}),                             # cvalid tail group, G = 25
    "dil2_17x19": (dc._case(2, 17, 19, 64, 0, 64, 2, ""), {}),                      # parity sub-lattices (ps = 2)
    "dil2_direct_12": (dc._case(2, 12, 12, 32, 0, 32, 2, ""), {}),                  # k_dw3_bwd_rows<2>
    "bns": (dc._case(2, 16, 16, 64, 0, 64, 1, "bns"), {}),
    "gate_dpool_adds": (dc._case(2, 16, 16, 64, 0, 64, 1, "ygate dpool add0 add1"), {}),
    "acc": (dc._case(2, 16, 16, 32, 0, 32, 1, "acc"), {}),
    "prior_dgamma": (dc._case(2, 16, 16, 32, 0, 32, 1, ""), {"prior": True, "pscale": 0.5}),
    "slice": (dc._case(2, 16, 16, 96, 32, 64, 1, "xgate"), {"sc": 72, "nogamma": True}),   # coff > 0, C_bn < cstride, padded statistics
    "s2_launcher": (dc._case(2, 16, 16, 32, 0, 32, 1, "", 3, 2), {}),                # k_dws2_bwd_lds: the launcher's own finalize call
    "gather_launcher": (dc._case(2, 4, 4, 64, 0, 64, 1, "acc"), {"prior": True}),   # W < 8: the row-gather pair
}
PW = {
    "64_64_8": (pc._case(64, 64, (2, 8, 8)), {}),
    "32_32_8": (pc._case(32, 32, (2, 8, 8)), {}),
    "128_128_16": (pc._case(128, 128, (2, 16, 16), "split"), {}),                    # (split: dz holds dy after the call)
    "64_128_16": (pc._case(64, 128, (2, 16, 16), "split dbias"), {"prior": True}),
    "128_64_16": (pc._case(128, 64, (2, 16, 16), "split acc"), {}),
    "64_64_9x7": (pc._case(64, 64, (2, 9, 7), "acc"), {"pscale": 0.25}),             # 126 pixels: no multiple of the 64-pixel tile
    "32_32_9x7": (pc._case(32, 32, (2, 9, 7), ""), {}),
    "32_32_bns": (pc._case(32, 32, (2, 8, 8), "bns"), {}),
    "64_64_views": (pc._case(64, 64, (2, 8, 8), "xgate ygate dpool acc views"), {"sc": 80, "nogamma": True}),
    "32_64_fallback": (pc._case(32, 64, (2, 8, 8), "dbias"), {"prior": True}),        # k_pw_bwd: the launcher's own finalize call
}
for _n, (_c, _) in DW.items():
    dc._ALL["finc_" + _n] = _c
for _n, (_c, _) in PW.items():
    pc._ALL["bwd"]["finc_" + _n] = _c


def _bn_inputs(c, count, extras, seed):
    """Sums as 32 replicas a backward leaves them (partial sums of count / 32 terms each), saved statistics, gamma, prior gradients."""
    sc = extras.get("sc", c)
    rng = np.random.Generator(np.random.PCG64(seed))
    b = {"sc": sc, "count": float(count), "pscale": extras.get("pscale", 1.0)}
    b["sums"] = torch.from_numpy(rng.standard_normal((32, 2, sc)) * (count / 32.0) ** 0.5 * 0.3)
    b["save"] = torch.from_numpy(np.stack([0.1 * rng.standard_normal(sc), 1 + 0.2 * np.abs(rng.standard_normal(sc))]).astype(np.float32))
    b["gamma"] = None if extras.get("nogamma") else torch.from_numpy((1 + 0.2 * rng.standard_normal(c)).astype(np.float32))
    pr = rng.standard_normal((2, c)).astype(np.float32) if extras.get("prior") else np.zeros((2, c), np.float32)
    b["dgamma"], b["dbeta"] = torch.from_numpy(pr[0].copy()), torch.from_numpy(pr[1].copy())
    return b


def _on(b, dev):
    return {k: (v.to(dev).clone() if torch.is_tensor(v) else v) for k, v in b.items()}


def _separate(b, coef, cs, coff, c):
    _lib.check(_lib.lib().lhn_bn_bwd_finalize2(_lib.ptr(b["sums"]), _lib.ptr(b["gamma"]), _lib.ptr(b["save"]), _lib.ptr(coef), cs, coff, c,
                                               b["sc"], C.c_double(b["count"]), _lib.ptr(b["dgamma"]), _lib.ptr(b["dbeta"]),
                                               C.c_float(b["pscale"]), _lib.stream()), "bn bwd finalize2")
    torch.cuda.synchronize()


def _src(b):
    f = BnBwdSrc()
    f.sums, f.save, f.gamma = b["sums"].data_ptr(), b["save"].data_ptr(), (b["gamma"].data_ptr() if b["gamma"] is not None else None)
    f.dgamma, f.dbeta = b["dgamma"].data_ptr(), b["dbeta"].data_ptr()
    f.count, f.pgrad_scale, f.stat_channels = b["count"], b["pscale"], b["sc"]
    return f


def _same_bits(a, b, what):
    a, b = a.detach().cpu().numpy() if torch.is_tensor(a) else a, b.detach().cpu().numpy() if torch.is_tensor(b) else b
    np.testing.assert_array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b,
                                  err_msg=what)


def _bars(name, got_by_path, r64, r32, rel_err, exact=()):
    bad = []
    for k, ref in r64.items():
        bar = max(TOL, 3 * rel_err(r32[k], ref))
        for path, got in got_by_path.items():
            err = rel_err(got[k], ref)
            print(f"bwd_fin_consumer {name} {path} {k}: err {err:.3e} bar {bar:.3e}")
            if not err <= bar:
                bad.append(f"{path} {k}: err {err:.3e} > bar {bar:.3e}")
    for path, got in got_by_path.items():
        bad += [f"{path} {k}: floats outside the outputs changed" for k, v in got.items() if k.endswith("_ok") and not bool(v)]
    for k in exact:
        _same_bits(got_by_path["new"][k], got_by_path["old"][k], f"{name} {k}")
    assert not bad, f"{name}: " + "; ".join(bad)


# ---------------------------------------------------------------- depthwise
def _dw_new(name, dev, g, b, coef):
    """dc.run with lhn_conv_dw_bwd4 in place of lhn_conv_dw_bwd / _bwd2 / _bwd3."""
    n, h, w, cs, coff, c, dil, _, k, stride, pad = dc._ALL[name]
    d = {kk: (v.to(dev) if torch.is_tensor(v) else v) for kk, v in g.items()}
    vx = dc._view(d["x"], coff, c, d["xtab"], d.get("xgate"))
    vy = dc._view(d["y"], coff, c, d["ytab"], d.get("ygate"))
    gv, dz = GradView(), d["dz"].clone()
    gv.dz, gv.dpool, gv.coef = dz.data_ptr(), (d["dpool"].data_ptr() if "dpool" in d else None), coef.data_ptr()
    nrep, rs = d["nrep"], c * k * k + dc.SLACK
    dwb = torch.zeros(nrep * rs, device=dev)
    dx = d["prior"].clone() if "prior" in d else torch.full((n, h, w, cs), 7.0, device=dev)
    before = d["prior"] if "prior" in d else torch.full_like(dx, 7.0)
    bs, sums = None, None
    if d["bns"]:
        sums = torch.zeros(32, 2, cs, dtype=torch.float64, device=dev)
        bs = pc.BnSum()
        bs.sums, bs.save, bs.C, bs.coff = sums.data_ptr(), d["save"].data_ptr(), cs, coff
    fs = _src(b)
    rc = _lib.lib().lhn_conv_dw_bwd4(C.byref(vx), _lib.ptr(d["w"].contiguous()), C.byref(vy), C.byref(gv), _lib.ptr(dx), int("prior" in d),
                                     _lib.ptr(dwb), k, stride, pad, dil, nrep, C.c_int64(rs), C.byref(bs) if bs is not None else None,
                                     _lib.ptr(d.get("add0")), _lib.ptr(d.get("add1")), C.byref(fs), _lib.stream())
    torch.cuda.synchronize()
    _lib.check(rc, "dw bwd4")
    out = {"dx": dx[..., coff:coff + c].cpu().numpy(), "dz_ok": np.array(torch.equal(dz, d["dz"])),
           "dx_outside_ok": np.array(torch.equal(torch.cat([dx[..., :coff], dx[..., coff + c:]], -1),
                                                 torch.cat([before[..., :coff], before[..., coff + c:]], -1))),
           "dw": dwb.view(nrep, rs)[:, :c * k * k].sum(0).view(c, k * k).cpu().numpy(),
           "dw_pad_ok": np.array(bool((dwb.view(nrep, rs)[:, c * k * k:] == 0).all()))}
    if sums is not None:
        out["sums"] = sums.sum(0)[:, coff:coff + c].cpu().numpy()
        out["sums_outside_ok"] = np.array(bool((torch.cat([sums[..., :coff], sums[..., coff + c:]], -1) == 0).all()))
    return out


@pytest.mark.parametrize("case", sorted(DW))
def test_dw_consumer_finalize_matches_separate_launch(dev, case):
    name, extras = "finc_" + case, DW[case][1]
    n, h, w, cs, coff, c, dil, _, k, stride, pad = dc._ALL[name]
    ho, wo = dc.out_hw(name)
    g = dc.inputs(name)
    bn = _bn_inputs(c, n * ho * wo, extras, 11)
    old_b, new_b = _on(bn, dev), _on(bn, dev)
    coef_old, coef_new = torch.full((3, cs), FILL, device=dev), torch.full((3, cs), FILL, device=dev)
    _separate(old_b, coef_old, cs, coff, c)
    old = dc.run(name, dev, dict(g, coef=coef_old))
    new = _dw_new(name, dev, g, new_b, coef_new)
    _same_bits(coef_new, coef_old, f"{name} coef")
    assert bool((coef_old[:, coff:coff + c] != FILL).all()) and bool((torch.cat([coef_old[:, :coff], coef_old[:, coff + c:]], 1) == FILL).all())
    _same_bits(new_b["dgamma"], old_b["dgamma"], f"{name} dgamma")
    _same_bits(new_b["dbeta"], old_b["dbeta"], f"{name} dbeta")
    assert torch.equal(new_b["sums"], bn["sums"].to(dev)), f"{name}: the sums were written"
    gref = dict(g, coef=coef_old.cpu())
    _bars(name, {"old": old, "new": new}, dc.reference(name, gref), dc.reference(name, gref, torch.float32), dc.rel_err, exact=("dx",))


# ---------------------------------------------------------------- 1x1
def _pw_new(name, dev, g, b, coef):
    """pc.run_bwd with lhn_conv_pw_bwd4 in place of lhn_conv_pw_bwd3 (NHWC cases)."""
    c = pc._ALL["bwd"][name]
    f, (n, h, w), cin, cout, stride = c["flags"], c["nhw"], c["cin"], c["cout"], c["stride"]
    xcs, xcoff, ycs, ycoff, ho, wo = pc.geometry("bwd", name)
    d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in g.items()}
    vx = pc._view(d["x"], xcoff, cin, d["xtab"], d.get("xgate"))
    vy = pc._view(d["y"], ycoff, cout, d["ytab"], d.get("ygate"))
    dz, gv = d["dz"].clone(), GradView()
    gv.dz, gv.dpool, gv.coef = dz.data_ptr(), (d["dpool"].data_ptr() if "dpool" in d else None), coef.data_ptr()
    nrep, rs = pc._nrep(c), cout * cin + cout + 16
    gbuf = torch.zeros(nrep, rs, device=dev)
    dbp = C.c_void_p(gbuf.data_ptr() + 4 * cout * cin) if "dbias" in f else None
    dx, acc = (d["prior"].clone(), 1) if "prior" in d else (torch.full((n, h, w, xcs), pc.PREFILL, device=dev), 0)
    o = pc.PwOpts()
    bs, sums = None, None
    if "bns" in f:
        sums = torch.zeros(32, 2, 128, dtype=torch.float64, device=dev)
        bs = pc.BnSum()
        bs.sums, bs.save, bs.C, bs.coff = sums.data_ptr(), d["save"].data_ptr(), 128, 64
    fs = _src(b)
    rc = _lib.lib().lhn_conv_pw_bwd4(C.byref(vx), _lib.ptr(d["w"].contiguous()), C.byref(vy), C.byref(gv), _lib.ptr(dx), acc, _lib.ptr(gbuf), dbp,
                                     stride, None, nrep, C.c_int64(rs), C.byref(o), C.byref(bs) if bs is not None else None, C.byref(fs),
                                     _lib.stream())
    torch.cuda.synchronize()
    _lib.check(rc, "pw bwd4")
    tot = gbuf.sum(0)
    before = d["prior"] if "prior" in d else torch.full_like(dx, pc.PREFILL)
    out = {"dw": tot[:cout * cin].view(cout, cin).cpu().numpy(), "dx": dx[..., xcoff:xcoff + cin].cpu().numpy(),
           "dw_pad_ok": np.array(bool((gbuf[:, cout * cin + (cout if dbp else 0):] == 0).all())),
           "dx_outside_ok": np.array(torch.equal(pc._outside(dx, xcoff, cin), pc._outside(before, xcoff, cin)))}
    if dbp:
        out["dbias"] = tot[cout * cin:cout * cin + cout].cpu().numpy()
    if "split" in f:
        out["dz"] = dz[..., ycoff:ycoff + cout].cpu().numpy()
        out["dz_outside_ok"] = np.array(torch.equal(pc._outside(dz, ycoff, cout), pc._outside(d["dz"], ycoff, cout)))
    else:
        out["dz_outside_ok"] = np.array(torch.equal(dz, d["dz"]))
    if sums is not None:
        t2 = sums.sum(0)[:, 64:64 + cin].cpu().numpy()
        out["sums_du"], out["sums_duxhat"] = t2[0], t2[1]
        out["sums_outside_ok"] = np.array(bool((pc._outside(sums, 64, cin) == 0).all()))
    return out


@pytest.mark.parametrize("case", sorted(PW))
def test_pw_consumer_finalize_matches_separate_launch(dev, case):
    name, extras = "finc_" + case, PW[case][1]
    c = pc._ALL["bwd"][name]
    (n, h, w), cout = c["nhw"], c["cout"]
    xcs, xcoff, ycs, ycoff, ho, wo = pc.geometry("bwd", name)
    g = pc.inputs("bwd", name)
    bn = _bn_inputs(cout, n * ho * wo, extras, 13)
    old_b, new_b = _on(bn, dev), _on(bn, dev)
    coef_old, coef_new = torch.full((3, ycs), FILL, device=dev), torch.full((3, ycs), FILL, device=dev)
    _separate(old_b, coef_old, ycs, ycoff, cout)
    old = pc.run_bwd(name, dev, dict(g, coef=coef_old))
    new = _pw_new(name, dev, g, new_b, coef_new)
    _same_bits(coef_new, coef_old, f"{name} coef")
    assert bool((coef_old[:, ycoff:ycoff + cout] != FILL).all()) and bool((pc._outside(coef_old, ycoff, cout) == FILL).all())
    _same_bits(new_b["dgamma"], old_b["dgamma"], f"{name} dgamma")
    _same_bits(new_b["dbeta"], old_b["dbeta"], f"{name} dbeta")
    assert torch.equal(new_b["sums"], bn["sums"].to(dev)), f"{name}: the sums were written"
    gref = dict(g, coef=coef_old.cpu())
    exact = ("dx", "dz") if "split" in c["flags"] else ("dx",)
    _bars(name, {"old": old, "new": new}, pc.reference_bwd(name, gref), pc.reference_bwd(name, gref, torch.float32), pc.rel_err, exact=exact)


# ---------------------------------------------------------------- the plan executor's switch, end to end
def test_train_step_is_bit_identical_with_and_without_the_switch(dev, tmp_path):
    res = []
    for mode in ("0", "1"):
        out = str(tmp_path / f"finc{mode}.npz")
        r = subprocess.run([sys.executable, os.path.join(HERE, "bwd_fin_child.py"), out],
                           env=dict(os.environ, LHN_BWD_FIN_CONSUMER=mode, LHN_DETERMINISTIC="1"), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        res.append(np.load(out))
    a, b = res
    assert set(a.files) == set(b.files) and any(k.startswith("g.") for k in a.files) and any(k.startswith("b.") for k in a.files)
    assert np.isfinite(a["loss"]) and float(np.abs(a["gflat"]).max()) > 0
    for k in a.files:
        _same_bits(a[k], b[k], k)
