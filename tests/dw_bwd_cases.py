"""Cases of the fused 3x3 depthwise backward (lhn_conv_dw_bwd / _bwd2 / _bwd3) run through the C ABI, with a float64 torch
reference.  Imported by tests/test_dw_bwd_gpu.py; run as a script (a child process with its own environment, e.g.
LHN_DW_BWD_V1=1 or LHN_DETERMINISTIC=1) it writes the kernel outputs of the named cases to an .npz file."""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from litehandnet_amd import _lib  # noqa: E402
from litehandnet_amd._lib import GradView, View  # noqa: E402

CASES = {
    # name: n, h, w, cstride, coff, c, dil, feature flags
    "bench_plain": (2, 64, 64, 64, 0, 64, 1, ""),
    "bench_bns": (2, 64, 64, 64, 0, 64, 1, "bns"),
    "bench_gy_dpool_acc": (2, 64, 64, 96, 32, 64, 1, "ygate dpool acc"),
    "bench_xgate_adds_nrep": (2, 64, 64, 64, 0, 64, 1, "xgate add0 add1 nrep"),
    "wide_plain": (2, 128, 128, 32, 0, 32, 1, "acc"),
    "wide_dpool_adds": (1, 128, 128, 32, 0, 32, 1, "ygate dpool add0"),
    "wide_bns": (1, 128, 128, 32, 0, 32, 1, "bns"),
    "parity_32": (2, 32, 32, 64, 0, 64, 2, "ygate dpool"),
    "parity_16_odd": (2, 16, 19, 64, 0, 64, 2, "xgate acc"),
    "dil2_narrow_8": (3, 8, 8, 64, 0, 64, 2, "ygate dpool acc"),
    "dil2_narrow_12": (2, 12, 12, 32, 0, 32, 2, "add0"),
    "small_8": (4, 8, 8, 128, 0, 128, 1, "ygate dpool"),
    "small_16_bns": (3, 16, 16, 64, 0, 64, 1, "bns"),
    "tail_20": (2, 16, 16, 40, 8, 20, 1, "xgate acc nrep"),
    "tail_40_parity": (2, 32, 32, 80, 40, 40, 2, "ygate dpool"),
    "tail_80_odd": (2, 15, 9, 80, 0, 80, 1, "add0 add1"),
}


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
    n, h, w, cs, coff, c, dil, flags = CASES[name]
    f = flags.split()
    g = {}
    g["x"] = _rand((n, h, w, cs), seed)
    g["y"] = _rand((n, h, w, cs), seed + 1)
    g["dz"] = _rand((n, h, w, cs), seed + 2)
    g["w"] = _rand((c, 9), seed + 3, 0.5)             # [C][9] of the view's channels
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
    for k in ("add0", "add1"):
        if k in f:
            g[k] = _rand((n, h, w, cs), seed + 15 + len(k) + (k == "add1"))
    if "bns" in f:
        g["save"] = torch.stack([0.1 * _rand((cs,), seed + 20), 1 + 0.2 * _rand((cs,), seed + 21).abs()]).contiguous()
    g["nrep"] = 4 if "nrep" in f else 1
    if os.environ.get("LHN_DETERMINISTIC") == "1":
        g["nrep"] = 16        # deterministic mode: one weight-gradient replica per workgroup of a channel group, as the plan runs it
    g["bns"] = "bns" in f
    return g


def run(name, dev, g=None):
    """The kernel's dx (channels of the view), dW (replicas summed) and, for BNS cases, the BatchNorm sums."""
    n, h, w, cs, coff, c, dil, _ = CASES[name]
    g = g or inputs(name)
    d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in g.items()}
    L, st = _lib.lib(), _lib.stream()
    vx = _view(d["x"], coff, c, d["xtab"], d.get("xgate"))
    vy = _view(d["y"], coff, c, d["ytab"], d.get("ygate"))
    gv = GradView()
    gv.dz, gv.dpool, gv.coef = d["dz"].data_ptr(), (d["dpool"].data_ptr() if "dpool" in d else None), d["coef"].data_ptr()
    nrep, rs = d["nrep"], c * 9 + 16
    dwb = torch.zeros(nrep * rs, device=dev)
    wbuf = d["w"].contiguous()
    dx = d["prior"].clone() if "prior" in d else torch.full((n, h, w, cs), 7.0, device=dev)
    acc = int("prior" in d)
    out = {}
    if d["bns"]:
        sums = torch.zeros(32, 2, cs, dtype=torch.float64, device=dev)
        _lib.check(L.lhn_conv_dw_bwd2(C.byref(vx), _lib.ptr(wbuf), C.byref(vy), C.byref(gv), _lib.ptr(dx), 0, _lib.ptr(dwb), 3, 1, dil, dil,
                                      nrep, C.c_int64(rs), _lib.ptr(sums), _lib.ptr(d["save"]), cs, coff, st), "dw bwd2")
        out["sums"] = sums.sum(0)[:, coff:coff + c].cpu().numpy()
    elif "add0" in d or "add1" in d:
        _lib.check(L.lhn_conv_dw_bwd3(C.byref(vx), _lib.ptr(wbuf), C.byref(vy), C.byref(gv), _lib.ptr(dx), acc, _lib.ptr(dwb), 3, 1, dil, dil,
                                      nrep, C.c_int64(rs), _lib.ptr(d.get("add0")), _lib.ptr(d.get("add1")), st), "dw bwd3")
    else:
        _lib.check(L.lhn_conv_dw_bwd(C.byref(vx), _lib.ptr(wbuf), C.byref(vy), C.byref(gv), _lib.ptr(dx), acc, _lib.ptr(dwb), 3, 1, dil, dil,
                                     nrep, C.c_int64(rs), st), "dw bwd")
    torch.cuda.synchronize()
    out["dx"] = dx[..., coff:coff + c].cpu().numpy()
    out["dx_outside"] = torch.cat([dx[..., :coff], dx[..., coff + c:]], -1).cpu().numpy()
    out["dw"] = dwb.view(nrep, rs)[:, :c * 9].sum(0).view(c, 9).cpu().numpy()
    return out


def reference(name, g=None):
    """float64: dy = A*du + B*y + C, then conv2d(groups=C) input / weight gradients; BNS sums of the producer."""
    n, h, w, cs, coff, c, dil, _ = CASES[name]
    g = g or inputs(name)
    sl = slice(coff, coff + c)
    dd = lambda t: t.double()  # noqa: E731
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
        slot = torch.tensor([[_seg(i, h) * 5 + _seg(j, w) for j in range(w)] for i in range(h)])
        e = e + dd(g["dpool"])[:, slot.view(-1), sl].view(n, h, w, c)
    u = y * ys + yh
    dy = A * (e * torch.where(u > 0, torch.ones_like(u), yl.expand_as(u))) + B * y + Cc
    wt = dd(g["w"]).view(c, 1, 3, 3)
    vxc, dyc = vx.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)
    dxv = torch.nn.grad.conv2d_input(vxc.shape, wt, dyc, padding=dil, dilation=dil, groups=c).permute(0, 2, 3, 1)
    dwv = torch.nn.grad.conv2d_weight(vxc, wt.shape, dyc, padding=dil, dilation=dil, groups=c).view(c, 9)
    out = {"dw": dwv.numpy()}
    dx = dxv.clone()
    if "prior" in g:
        dx = dx + dd(g["prior"])[..., sl]
    for k in ("add0", "add1"):
        if k in g:
            dx = dx + dd(g[k])[..., sl]
    out["dx"] = dx.numpy()
    if g["bns"]:
        mean, inv = dd(g["save"][0, sl]), dd(g["save"][1, sl])
        du = dxv * torch.where(ux > 0, torch.ones_like(ux), xl.expand_as(ux))
        out["sums"] = torch.stack([du.sum((0, 1, 2)), (du * (x - mean) * inv).sum((0, 1, 2))]).numpy()
    return out


if __name__ == "__main__":
    # child: python tests/dw_bwd_cases.py OUT.npz REPEATS CASE...
    dst, reps, names = sys.argv[1], int(sys.argv[2]), sys.argv[3:]
    dev = torch.device("cuda:0")
    res = {}
    for nm in names:
        for r in range(reps):
            for k, v in run(nm, dev).items():
                res[f"{nm}/{r}/{k}"] = v
    np.savez(dst, **res)
