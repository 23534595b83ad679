"""Cases of the depthwise backward (lhn_conv_dw_bwd / _bwd2 / _bwd3: the fused 3x3 kernels, the 7x7 tile kernel, the stride-2
kernel and the row-gather pair) run through the C ABI, with a plain torch reference on the CPU (float64, or float32 to measure
what the same operation loses in the kernels' own precision).  Imported by tests/test_dw_bwd_gpu.py; run as a script (a child
process with its own environment, e.g. LHN_DW_BWD_V1=1, LHN_DW_GATHER=1 or LHN_DETERMINISTIC=1) it writes the kernel outputs of
the named cases to an .npz file.

kernel_of(name) asks the library which kernels a case runs (lhn_conv_dw_route); profiles/dw_instances.md is printed from it."""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from litehandnet_amd import _lib  # noqa: E402
from litehandnet_amd._lib import GradView, View  # noqa: E402

def _case(n, h, w, cs, coff, c, dil, flags, k=3, stride=1, pad=None):
    return (n, h, w, cs, coff, c, dil, flags, k, stride, dil * (k - 1) // 2 if pad is None else pad)


CASES = {
    # name: n, h, w, cstride, coff, c, dil, feature flags [, k = 3, stride = 1, pad = "same"]
    "bench_plain": _case(2, 64, 64, 64, 0, 64, 1, ""),
    "bench_bns": _case(2, 64, 64, 64, 0, 64, 1, "bns"),
    "bench_gy_dpool_acc": _case(2, 64, 64, 96, 32, 64, 1, "ygate dpool acc"),
    "bench_xgate_adds_nrep": _case(2, 64, 64, 64, 0, 64, 1, "xgate add0 add1 nrep"),
    "wide_plain": _case(2, 128, 128, 32, 0, 32, 1, "acc"),
    "wide_dpool_adds": _case(1, 128, 128, 32, 0, 32, 1, "ygate dpool add0"),
    "wide_bns": _case(1, 128, 128, 32, 0, 32, 1, "bns"),
    "parity_32": _case(2, 32, 32, 64, 0, 64, 2, "ygate dpool"),
    "parity_16_odd": _case(2, 16, 19, 64, 0, 64, 2, "xgate acc"),
    "dil2_narrow_8": _case(3, 8, 8, 64, 0, 64, 2, "ygate dpool acc"),
    "dil2_narrow_12": _case(2, 12, 12, 32, 0, 32, 2, "add0"),
    "small_8": _case(4, 8, 8, 128, 0, 128, 1, "ygate dpool"),
    "small_16_bns": _case(3, 16, 16, 64, 0, 64, 1, "bns"),
    "tail_20": _case(2, 16, 16, 40, 8, 20, 1, "xgate acc nrep"),
    "tail_40_parity": _case(2, 32, 32, 80, 40, 40, 2, "ygate dpool"),
    "tail_80_odd": _case(2, 15, 9, 80, 0, 80, 1, "add0 add1"),
    # k_dws2_bwd_lds: 3x3, stride 2, pad 1 (every input pixel belongs to one tile, the last row / column of even maps included)
    "s2_16": _case(2, 16, 16, 64, 0, 64, 1, "", 3, 2),
    "s2_17x19": _case(2, 17, 19, 32, 0, 32, 1, "xgate acc", 3, 2),
    "s2_9_tail20": _case(1, 9, 9, 40, 8, 20, 1, "ygate dpool", 3, 2),
    "s2_34x66": _case(2, 34, 66, 32, 0, 32, 1, "nrep", 3, 2),
    # k_dwk_bwd_lds<7,1>
    "k7_16": _case(2, 16, 16, 32, 0, 32, 1, "", 7),
    "k7_9x21_tail40": _case(1, 9, 21, 40, 0, 40, 1, "xgate acc nrep", 7),
    "k7_12x17_dpool": _case(2, 12, 17, 64, 0, 64, 1, "ygate dpool", 7),
    "k7_16_adds": _case(2, 16, 16, 32, 0, 32, 1, "add0 add1", 7),
    # the row-gather pair k_dw_bwd_data + k_dw_bwd_weight, reached by shape
    "g3_4x4_acc": _case(2, 4, 4, 64, 0, 64, 1, "acc"),
    "g3_4x4_dpool": _case(2, 4, 4, 64, 0, 64, 1, "ygate dpool"),
    "g3_7x5_acc": _case(2, 7, 5, 64, 0, 64, 1, "acc"),
    "g3_7x5_dpool": _case(2, 7, 5, 64, 0, 64, 1, "ygate dpool"),
    "g1_w": _case(2, 9, 9, 32, 0, 32, 1, "", 1),
    "g1_identity": _case(2, 9, 9, 32, 0, 32, 1, "wnull", 1),                # w = dw = NULL: dx only
    "g7_6x6": _case(2, 6, 6, 32, 0, 32, 1, "", 7),                          # seven weight launches
    "g3_valid": _case(2, 10, 10, 32, 0, 32, 1, "", 3, 1, 0),
    "g3_c20": _case(2, 5, 7, 40, 8, 20, 1, "xgate"),
    "g3_nrep": _case(3, 4, 6, 64, 0, 64, 1, "nrep"),
}
NEW_PREFIXES = ("s2_", "k7_", "g1_", "g3_", "g7_")

# calls the library must refuse (non-zero status, the reason in lhn_last_error, nothing written): case, reason
REFUSE = {
    "k5": (_case(2, 16, 16, 32, 0, 32, 1, "", 5), "k=5"),
    "bns_acc": (_case(2, 16, 16, 32, 0, 32, 1, "bns acc"), "fused BatchNorm sums need"),
    "bns_xgate": (_case(2, 16, 16, 32, 0, 32, 1, "bns xgate"), "fused BatchNorm sums need"),
    "bns_k7": (_case(2, 16, 16, 32, 0, 32, 1, "bns", 7), "built for the 3x3 / dilation 1 kernel"),
    "bns_dil2": (_case(2, 16, 16, 32, 0, 32, 2, "bns"), "built for the 3x3 / dilation 1 kernel"),
    "bns_w4": (_case(2, 4, 4, 32, 0, 32, 1, "bns"), "fused BatchNorm sums need"),
    "adds_w4": (_case(2, 4, 4, 32, 0, 32, 1, "add0"), "gradient addends need"),
}
_ALL = dict(CASES, **{k: v[0] for k, v in REFUSE.items()})


def out_hw(name):
    n, h, w, cs, coff, c, dil, _, k, stride, pad = _ALL[name]
    f = lambda e: (e + 2 * pad - dil * (k - 1) - 1) // stride + 1      # noqa: E731
    return f(h), f(w)


F_NO_WEIGHT, F_BNSUM, F_ADDS, F_DX_ACC = 1, 4, 8, 64        # LHN_DW_F_* (include/lhn.h)
SW_GATHER, SW_BWD_V1, SW_BWD_SMALL = 1, 2, 4                # LHN_DW_SW_*


def kernel_of(name, gather=False, v1=False, small=True):
    """The kernels lhn_conv_dw_bwd / _bwd2 / _bwd3 launch for a case, asked of the library (lhn_conv_dw_route: host only).
    gather: LHN_DW_GATHER=1, v1: LHN_DW_BWD_V1=1, small=False: LHN_DW_BWD_SMALL=0.  None: no kernel for the case."""
    n, h, w, cs, coff, c, dil, flags, k, stride, pad = _ALL[name]
    f = flags.split()
    feat = (F_NO_WEIGHT * ("wnull" in f) | F_BNSUM * ("bns" in f) | F_ADDS * ("add0" in f or "add1" in f) | F_DX_ACC * ("acc" in f))
    r = _lib.lib().lhn_conv_dw_route(1, h, w, c, k, stride, pad, dil, feat, SW_GATHER * gather | SW_BWD_V1 * v1 | SW_BWD_SMALL * small)
    return r.decode() if r is not None else None


def _rand(shape, seed, scale=1.0):
    return torch.from_numpy((np.random.Generator(np.random.PCG64(seed)).standard_normal(shape) * scale).astype(np.float32))


def _view(t, coff, c, table=None, gate=None):
    v = View()
    v.data, v.table, v.gate, v.pend = t.data_ptr(), (table.data_ptr() if table is not None else None), \
        (gate.data_ptr() if gate is not None else None), None
    v.N, v.H, v.W, v.cstride, v.coff, v.C = t.shape[0], t.shape[1], t.shape[2], t.shape[3], coff, c
    return v


def _seg(h, s):
    lo = lambda i: (i * s) // 3             # noqa: E731
    hi = lambda i: ((i + 1) * s + 2) // 3   # noqa: E731
    return int(h >= lo(1)) + int(h >= hi(0)) + int(h >= lo(2)) + int(h >= hi(1))


def inputs(name, seed=7):
    n, h, w, cs, coff, c, dil, flags, k, stride, pad = _ALL[name]
    ho, wo = out_hw(name)
    f = flags.split()
    g = {}
    g["x"] = _rand((n, h, w, cs), seed)
    g["y"] = _rand((n, ho, wo, cs), seed + 1)
    g["dz"] = _rand((n, ho, wo, cs), seed + 2)
    if "wnull" not in f:
        g["w"] = _rand((c, k * k), seed + 3, 1.5 / k)             # [C][k*k] of the view's channels (0.5 for the 3x3)
    tab = lambda s: torch.stack([1 + 0.3 * _rand((cs,), s), 0.2 * _rand((cs,), s + 1), torch.full((cs,), 0.1)]).contiguous()  # noqa: E731
    g["xtab"], g["ytab"] = tab(seed + 4), tab(seed + 6)
    g["coef"] = torch.stack([1 + 0.2 * _rand((cs,), seed + 8), 0.1 * _rand((cs,), seed + 9), 0.1 * _rand((cs,), seed + 10)]).contiguous()
    if "xgate" in f:
        g["xgate"] = torch.sigmoid(_rand((n, cs), seed + 11))
    if "ygate" in f:
        g["ygate"] = torch.sigmoid(_rand((n, cs), seed + 12))
    if "dpool" in f:
        g["dpool"] = 0.3 * _rand((n, 25, cs), seed + 13)
    if "acc" in f:
        g["prior"] = _rand((n, h, w, cs), seed + 14)
    for kk in ("add0", "add1"):
        if kk in f:
            g[kk] = _rand((n, h, w, cs), seed + 15 + len(kk) + (kk == "add1"))
    if "bns" in f:
        g["save"] = torch.stack([0.1 * _rand((cs,), seed + 20), 1 + 0.2 * _rand((cs,), seed + 21).abs()]).contiguous()
    g["nrep"] = 4 if "nrep" in f else 1
    if os.environ.get("LHN_DETERMINISTIC") == "1":
        g["nrep"] = 16        # deterministic mode: one weight-gradient replica per workgroup of a channel group, as the plan runs it
    g["bns"] = "bns" in f
    return g


SLACK = 16          # floats behind every weight-gradient replica: must stay zero


def run(name, dev, g=None, expect_fail=False):
    """The kernel's dx (channels of the view), dW (replicas summed) and, for BNS cases, the BatchNorm sums; `*_ok` flags: floats
    that must keep their bits did."""
    n, h, w, cs, coff, c, dil, _, k, stride, pad = _ALL[name]
    g = g or inputs(name)
    d = {kk: (v.to(dev) if torch.is_tensor(v) else v) for kk, v in g.items()}
    L, st = _lib.lib(), _lib.stream()
    vx = _view(d["x"], coff, c, d["xtab"], d.get("xgate"))
    vy = _view(d["y"], coff, c, d["ytab"], d.get("ygate"))
    gv = GradView()
    dz = d["dz"].clone()
    gv.dz, gv.dpool, gv.coef = dz.data_ptr(), (d["dpool"].data_ptr() if "dpool" in d else None), d["coef"].data_ptr()
    nrep, rs = d["nrep"], c * k * k + SLACK
    dwb = torch.zeros(nrep * rs, device=dev) if "w" in d else None
    wbuf = d["w"].contiguous() if "w" in d else None
    dx = d["prior"].clone() if "prior" in d else torch.full((n, h, w, cs), 7.0, device=dev)
    acc = int("prior" in d)
    out = {}
    sums = None
    geo = (k, stride, pad, dil)
    if d["bns"]:
        sums = torch.zeros(32, 2, cs, dtype=torch.float64, device=dev)
        rc = L.lhn_conv_dw_bwd2(C.byref(vx), _lib.ptr(wbuf), C.byref(vy), C.byref(gv), _lib.ptr(dx), acc, _lib.ptr(dwb), *geo,
                                nrep, C.c_int64(rs), _lib.ptr(sums), _lib.ptr(d["save"]), cs, coff, st)
        what = "dw bwd2"
    elif "add0" in d or "add1" in d:
        rc = L.lhn_conv_dw_bwd3(C.byref(vx), _lib.ptr(wbuf), C.byref(vy), C.byref(gv), _lib.ptr(dx), acc, _lib.ptr(dwb), *geo,
                                nrep, C.c_int64(rs), _lib.ptr(d.get("add0")), _lib.ptr(d.get("add1")), st)
        what = "dw bwd3"
    else:
        rc = L.lhn_conv_dw_bwd(C.byref(vx), _lib.ptr(wbuf), C.byref(vy), C.byref(gv), _lib.ptr(dx), acc, _lib.ptr(dwb), *geo,
                               nrep, C.c_int64(rs), st)
        what = "dw bwd"
    torch.cuda.synchronize()
    before = d["prior"] if "prior" in d else torch.full_like(dx, 7.0)
    if expect_fail:
        return rc, torch.equal(dx, before) and bool((dwb == 0).all()) and torch.equal(dz, d["dz"]) and (sums is None or bool((sums == 0).all()))
    _lib.check(rc, what)
    if sums is not None:
        out["sums"] = sums.sum(0)[:, coff:coff + c].cpu().numpy()
        out["sums_outside_ok"] = np.array(bool((torch.cat([sums[..., :coff], sums[..., coff + c:]], -1) == 0).all()))
    out["dx"] = dx[..., coff:coff + c].cpu().numpy()
    out["dx_outside"] = torch.cat([dx[..., :coff], dx[..., coff + c:]], -1).cpu().numpy()
    out["dx_outside_ok"] = np.array(torch.equal(torch.cat([dx[..., :coff], dx[..., coff + c:]], -1),
                                                torch.cat([before[..., :coff], before[..., coff + c:]], -1)))
    out["dz_ok"] = np.array(torch.equal(dz, d["dz"]))             # the depthwise backward only reads dz
    if dwb is not None:
        out["dw"] = dwb.view(nrep, rs)[:, :c * k * k].sum(0).view(c, k * k).cpu().numpy()
        out["dw_pad_ok"] = np.array(bool((dwb.view(nrep, rs)[:, c * k * k:] == 0).all()))
    return out


def reference(name, g=None, dtype=torch.float64):
    """dy = A*du + B*y + C, then conv2d(groups=C) input / weight gradients; BNS sums of the producer.  dpool segments are taken
    on y's geometry."""
    n, h, w, cs, coff, c, dil, _, k, stride, pad = _ALL[name]
    ho, wo = out_hw(name)
    g = g or inputs(name)
    sl = slice(coff, coff + c)
    dd = lambda t: t.to(dtype)  # noqa: E731
    x, y, dz = dd(g["x"])[..., sl], dd(g["y"])[..., sl], dd(g["dz"])[..., sl]
    xs, xh, xl = (dd(g["xtab"][i, sl]) for i in range(3))
    ys, yh, yl = (dd(g["ytab"][i, sl]) for i in range(3))
    A, B, Cc = (dd(g["coef"][i, sl]) for i in range(3))
    ux = x * xs + xh
    vx = torch.where(ux > 0, ux, ux * xl)
    if "xgate" in g:
        vx = vx * dd(g["xgate"])[:, None, None, sl]
    e = dz * (dd(g["ygate"])[:, None, None, sl] if "ygate" in g else 1.0)
    if "dpool" in g:
        slot = torch.tensor([[_seg(i, ho) * 5 + _seg(j, wo) for j in range(wo)] for i in range(ho)])
        e = e + dd(g["dpool"])[:, slot.view(-1), sl].view(n, ho, wo, c)
    u = y * ys + yh
    dy = A * (e * torch.where(u > 0, torch.ones_like(u), yl.expand_as(u))) + B * y + Cc
    wt = dd(g["w"]).view(c, 1, k, k) if "w" in g else torch.ones(c, 1, 1, 1, dtype=dtype)
    vxc, dyc = vx.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)
    dxv = torch.nn.grad.conv2d_input(vxc.shape, wt, dyc, stride=stride, padding=pad, dilation=dil, groups=c).permute(0, 2, 3, 1)
    out = {}
    if "w" in g:
        out["dw"] = torch.nn.grad.conv2d_weight(vxc, wt.shape, dyc, stride=stride, padding=pad, dilation=dil, groups=c).view(c, k * k).double().numpy()
    dx = dxv.clone()
    if "prior" in g:
        dx = dx + dd(g["prior"])[..., sl]
    for kk in ("add0", "add1"):
        if kk in g:
            dx = dx + dd(g[kk])[..., sl]
    out["dx"] = dx.double().numpy()
    if g["bns"]:
        mean, inv = dd(g["save"][0, sl]), dd(g["save"][1, sl])
        du = dxv * torch.where(ux > 0, torch.ones_like(ux), xl.expand_as(ux))
        out["sums"] = torch.stack([du.sum((0, 1, 2)), (du * (x - mean) * inv).sum((0, 1, 2))]).double().numpy()
    return out


def rel_err(a, b):
    """Max absolute difference over every element, relative to the reference's largest magnitude."""
    return float(np.abs(np.asarray(a, np.float64) - b).max()) / max(float(np.abs(b).max()), 1e-30)


def _check_reference():
    import time
    t0, worst = time.time(), 0.0
    for nm in CASES:
        g = inputs(nm)
        r64, r32 = reference(nm, g), reference(nm, g, torch.float32)
        for kk in r64:
            assert np.isfinite(r64[kk]).all() and np.abs(r64[kk]).max() > 0, f"{nm} {kk}: reference not finite or all zeros"
            e = rel_err(r32[kk], r64[kk])
            assert np.isfinite(3 * e), f"{nm} {kk}"
            worst = max(worst, e)
        print(f"{nm:22s} {kernel_of(nm):50s} small=0: {kernel_of(nm, small=False):50s} v1: {kernel_of(nm, v1=True):50s} "
              f"gather: {kernel_of(nm, gather=True)}")
    print(f"{len(CASES)} cases, worst float32 error {worst:.2e}, {time.time() - t0:.1f} s")


if __name__ == "__main__":
    # child: python tests/dw_bwd_cases.py OUT.npz REPEATS CASE...   |   python tests/dw_bwd_cases.py --check-reference  (CPU only)
    if sys.argv[1] == "--check-reference":
        _check_reference()
        sys.exit(0)
    dst, reps, names = sys.argv[1], int(sys.argv[2]), sys.argv[3:]
    dev = torch.device("cuda:0")
    res = {}
    for nm in names:
        for r in range(reps):
            for k, v in run(nm, dev).items():
                res[f"{nm}/{r}/{k}"] = v
    np.savez(dst, **res)
