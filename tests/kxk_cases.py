"""Cases of the dense 3x3 convolution (lhn_conv_kxk_fwd / lhn_conv_kxk_bwd, csrc/k_conv_kxk.hip) run through the C ABI, with a
plain torch reference on the CPU (float64, or float32 to measure what the same operation loses in the kernels' own precision).
Imported by tests/test_kxk_gpu.py; run as a script (a child process with its own environment: LHN_DETERMINISTIC=1, LHN_PLAIN=0/1)
it writes the kernel outputs of the named cases to an .npz file:
    python tests/kxk_cases.py OUT.npz REPEATS fwd:NAME bwd:NAME ...
    python tests/kxk_cases.py --check-reference        (CPU only: every case's inputs and both references)

    python tests/kxk_cases.py --instances              (CPU only: prints profiles/kxk_instances.md)
kernel_of(kind, name) asks the library which kernels a case launches (lhn_conv_kxk_route: host only); which case reaches which
template instantiation, by default, in the deterministic child (2 CUs) and under LHN_PLAIN=0 / 1, is profiles/kxk_instances.md."""
import ctypes as C
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pw_cases import PREFILL, GradView, _dact, _kinks, _lib, _nrep, _outside, _rand, _seg, _tab, _value, _view, rel_err  # noqa: E402,F401

PAIRS = [(ci, co) for ci in (32, 64, 128) for co in (32, 64, 128)]
SLACK = 16                      # floats behind every gradient replica and behind the weight scratch: must keep their fill


def _case(cin, cout, nhw, flags="", stride=1, **kw):
    return dict(cin=cin, cout=cout, nhw=nhw, flags=flags.split(), stride=stride, **kw)


# ---------------------------------------------------------------- forward table
# flags: xtab / xgate: pending transform / gate on x;  xview: x is channels [64, 64 + Cin) of a wider buffer;  yview: y is channels
# [32, 32 + Cout) of a wider buffer;  nostats.  Every case runs with the tap-major weight scratch unless the caller says wt=False.
FWD = {}
for _ci, _co in PAIRS:
    FWD[f"pair_{_ci}_{_co}"] = _case(_ci, _co, (3, 9, 13), "xtab")                  # 351 px: no multiple of the 128-pixel tile, images straddle tiles
FWD["tiny_64_64"] = _case(64, 64, (1, 5, 7))                                        # 35 px: under one tile
FWD["tiny_32_128"] = _case(32, 128, (1, 5, 7))
FWD["view_64_64"] = _case(64, 64, (2, 12, 20), "xtab xgate xview yview")
FWD["view_128_32"] = _case(128, 32, (2, 12, 20), "xtab xgate xview yview")
for _ci, _co in ((128, 64), (64, 64), (32, 32)):
    FWD[f"s2_{_ci}_{_co}_odd"] = _case(_ci, _co, (2, 11, 11), "xtab", stride=2)
    FWD[f"s2_{_ci}_{_co}_even"] = _case(_ci, _co, (1, 8, 10), "xtab", stride=2)
FWD["nostats_64_64"] = _case(64, 64, (3, 9, 13), "xtab nostats")
for _ci, _co in ((64, 40), (32, 48), (128, 40)):                                    # the last feature tile is 8 / 16 channels wide
    FWD[f"tail_{_ci}_{_co}"] = _case(_ci, _co, (2, 9, 11), "xtab")
for _ci, _co in PAIRS:
    FWD[f"mt_{_ci}_{_co}"] = _case(_ci, _co, (3, 24, 25), "xtab")                   # 1,800 px = 15 tiles: the deterministic child's NT = Cout / 32
FWD["big_128_128"] = _case(128, 128, (1, 257, 257), "xtab")                         # 517 tiles: NT = 4, more tiles than resident workgroups
FWD["big_32_32"] = _case(32, 32, (2, 257, 257), "xtab")                             # 1,033 tiles

# ---------------------------------------------------------------- backward table
# always: x table, y table, coef, 4 weight-gradient replicas (nrep=...), dx prefilled 7.0, weight scratch.  flags: acc: dx holds a
# prior and is added to;  xgate / ygate / dpool;  views: x / dx are channels [64, 64 + Cin), y / dz channels [32, 32 + Cout) of wider
# buffers;  nodx
BWD = {}
for _i, (_ci, _co) in enumerate(PAIRS):
    BWD[f"pair_{_ci}_{_co}"] = _case(_ci, _co, (3, 9, 13), "acc" if _i % 2 else "")
for _i, (_ci, _co) in enumerate(PAIRS):
    BWD[f"rep1_{_ci}_{_co}"] = _case(_ci, _co, (3, 9, 13), "" if _i % 2 else "acc", nrep=1)      # adds straight into dw; no cosplit
for _ci, _co in ((64, 64), (64, 128), (128, 64), (128, 128)):
    BWD[f"cosplit_{_ci}_{_co}"] = _case(_ci, _co, (4, 31, 33), "")                  # 4,092 px = 64 wgrad tiles = 16 * nrep: 16 tiles per block, exclusive flush
BWD["nocosplit_64_64"] = _case(64, 64, (5, 29, 29), "acc")                          # 4,205 px = 66 tiles: one past the threshold, atomic flush
BWD["full_64_64"] = _case(64, 64, (2, 16, 19), "ygate dpool acc views")
BWD["full_32_128"] = _case(32, 128, (2, 16, 19), "ygate dpool acc views")
BWD["dpool_32_32"] = _case(32, 32, (2, 16, 19), "dpool")                            # a pooled gradient forces the plain path below 4096
BWD["xgate_64_64"] = _case(64, 64, (3, 9, 13), "xgate")
BWD["fly_32_64"] = _case(32, 64, (2, 16, 19), "xgate ygate acc views")              # dy on the fly (lhn_dy_fast) with a gate, in views
BWD["fly_64_32"] = _case(64, 32, (2, 16, 19), "ygate views")
BWD["nodx_64_64"] = _case(64, 64, (2, 8, 8), "nodx")
BWD["nodx_128_128"] = _case(128, 128, (2, 8, 8), "nodx")
for _ci, _co in ((128, 64), (32, 32)):
    for _e, _nhw in (("odd", (2, 11, 11)), ("even", (1, 8, 10))):
        BWD[f"s2_{_ci}_{_co}_{_e}_store"] = _case(_ci, _co, _nhw, "", stride=2)
        BWD[f"s2_{_ci}_{_co}_{_e}_acc"] = _case(_ci, _co, _nhw, "acc", stride=2)
for _ci, _co in PAIRS:
    BWD[f"mt_{_ci}_{_co}"] = _case(_ci, _co, (3, 24, 25), "acc" if _ci == _co else "")
BWD["big_128_128"] = _case(128, 128, (1, 257, 257), "", nrep=16)                    # dgrad NT = 4, wgrad <128, 4> with the atomic flush

# calls the library must refuse (non-zero status, an error text, nothing written: y / dx / dW / scratch keep their fill, dz its bits)
FWD_REFUSE = {
    "r_64_96": _case(64, 96, (2, 8, 8), "xtab", refuse="unsupported channels"),                          # three feature tiles
    "r_48_64": _case(48, 64, (2, 8, 8), "xtab", refuse="unsupported channels"),
    "r_geometry": _case(64, 64, (2, 8, 8), "xtab badgeo", refuse="geometry / stride"),                   # y one row too tall
    "r_stride3": _case(64, 64, (2, 9, 9), "xtab", stride=3, refuse="geometry / stride 3"),
}
BWD_REFUSE = {
    "r_48_64": _case(48, 64, (2, 8, 8), "", refuse="unsupported channels"),                              # a dgrad instance exists, no wgrad
    "r_128_96": _case(128, 96, (2, 8, 8), "", refuse="unsupported channels"),
    "r_96_64": _case(96, 64, (2, 8, 8), "", refuse="unsupported channels"),
    "r_stride3": _case(64, 64, (2, 9, 9), "", stride=3, refuse="geometry / stride 3"),
}
TABLES = {"fwd": FWD, "bwd": BWD}
_ALL = {"fwd": dict(FWD, **FWD_REFUSE), "bwd": dict(BWD, **BWD_REFUSE)}


def geometry(kind, name):
    """Buffer widths and channel offsets of a case: (xcs, xcoff, ycs, ycoff, Ho, Wo)."""
    c = _ALL[kind][name]
    f, (n, h, w) = c["flags"], c["nhw"]
    wide_x, wide_y = ("xview" in f or "views" in f), ("yview" in f or "views" in f)
    xcs, xcoff = (c["cin"] + 64, 64) if wide_x else (c["cin"], 0)
    ycs, ycoff = (c["cout"] + 32, 32) if wide_y else (c["cout"], 0)
    s = c["stride"]
    return xcs, xcoff, ycs, ycoff, (h - 1) // s + 1 + int("badgeo" in f), (w - 1) // s + 1


def plain_path(c):
    """Whether lhn_conv_kxk_bwd turns dz into dy in place for this case, under this process's environment (as the library's
    getenv sees it: a variable that is set but empty is set, and is not '1').  The harness's own statement of the rule;
    tests/test_kxk_route_cpu.py holds it against the library's answer for every case and setting."""
    pe = os.environ.get("LHN_PLAIN")
    return ("dpool" in c["flags"] or max(c["cin"], c["cout"]) > 128 or
            (pe[:1] == "1" if pe is not None else c["cin"] * c["cout"] >= 64 * 64))


# LHN_KXK_F_* / LHN_KXK_SW_* (include/lhn.h)
F_DX, F_DPOOL, F_WT = 1, 2, 4
SW_PLAIN0, SW_PLAIN1 = 1, 2
# the settings a table of profiles/kxk_instances.md is printed for: title, kernel_of keywords
SETTINGS = (("default dispatch on 256 CUs", {}), ("`LHN_DETERMINISTIC=1` (2 CUs, 16 gradient replicas)", {"cus": 2}),
            ("`LHN_PLAIN=0`", {"plain": 0}), ("`LHN_PLAIN=1`", {"plain": 1}))


def kernel_of(kind, name, cus=256, plain=None, wt=True):
    """The launches of lhn_conv_kxk_fwd / lhn_conv_kxk_bwd for a case (of this module or of kxk256_cases, once imported), in order,
    asked of the library (lhn_conv_kxk_route: host only).  cus: the compute units the grids are sized for; 2 is deterministic mode,
    in which run_bwd passes 16 gradient replicas (_nrep).  plain: LHN_PLAIN=0 / 1, None = unset.  None: no kernel for the case."""
    c = _ALL[kind][name]
    n, h, w = c["nhw"]
    feat = F_WT * wt | (F_DX * ("nodx" not in c["flags"]) | F_DPOOL * ("dpool" in c["flags"]) if kind == "bwd" else 0)
    sw = 0 if plain is None else (SW_PLAIN1 if int(plain) == 1 else SW_PLAIN0)
    r = _lib.lib().lhn_conv_kxk_route(int(kind == "bwd"), n, h, w, c["cin"], c["cout"], c["stride"], 16 if cus == 2 else c.get("nrep", 4),
                                      feat, cus, sw)
    return r.decode() if r is not None else None


def _gen(kind, name, seed):
    c = _ALL[kind][name]
    f, (n, h, w), cin, cout = c["flags"], c["nhw"], c["cin"], c["cout"]
    xcs, xcoff, ycs, ycoff, ho, wo = geometry(kind, name)
    g = {"seed": seed}
    g["x"] = _rand((n, h, w, xcs), seed)
    g["w"] = _rand((cout, cin, 3, 3), seed + 3, (9 * cin) ** -0.5)
    if kind == "bwd" or "xtab" in f:
        g["xtab"] = _tab(xcs, seed + 4)
    if "xgate" in f:
        g["xgate"] = torch.sigmoid(_rand((n, xcs), seed + 11))
    if kind == "fwd":
        return g
    g["y"] = _rand((n, ho, wo, ycs), seed + 1)
    g["ytab"] = _tab(ycs, seed + 6)
    g["dz"] = _rand((n, ho, wo, ycs), seed + 2)
    g["coef"] = torch.stack([1 + 0.2 * _rand((ycs,), seed + 8), 0.1 * _rand((ycs,), seed + 9), 0.1 * _rand((ycs,), seed + 10)]).contiguous()
    if "ygate" in f:
        g["ygate"] = torch.sigmoid(_rand((n, ycs), seed + 12))
    if "dpool" in f:
        g["dpool"] = 0.3 * _rand((n, 25, ycs), seed + 13)
    if "acc" in f:
        g["prior"] = _rand((n, h, w, xcs), seed + 14)
    return g


def inputs(kind, name, seed=7):
    """Seeded inputs; a seed at which some activation input changes sign between float32 and float64 is passed over."""
    for s in range(seed, seed + 1000, 100):
        g = _gen(kind, name, s)
        if sum(_kinks(g[k], g[k + "tab"]) for k in ("x", "y") if k in g and k + "tab" in g) == 0:
            return g
    raise AssertionError(f"{kind}:{name}: no seed without an activation kink")


def _scratch(c, dev, wt):
    return torch.full((9 * c["cout"] * c["cin"] + SLACK,), PREFILL, device=dev) if wt else None


# ---------------------------------------------------------------- kernels
def run_fwd(name, dev, g=None, stats=None, wt=True, expect_fail=False):
    """Outputs of lhn_conv_kxk_fwd as numpy arrays (the view's channels), plus `*_ok` flags: every float outside the views still
    holds its prefill, bit for bit, and the tap-major scratch holds wt[tap][co][ci] = w[co][ci][tap] and its slack.  stats=False
    switches the statistics off for a case that has them; wt=False passes wt_scratch = NULL."""
    c = _ALL["fwd"][name]
    f, (n, h, w), cin, cout, stride = c["flags"], c["nhw"], c["cin"], c["cout"], c["stride"]
    xcs, xcoff, ycs, ycoff, ho, wo = geometry("fwd", name)
    g = g or inputs("fwd", name)
    d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in g.items()}
    L, st = _lib.lib(), _lib.stream()
    with_stats = ("nostats" not in f) if stats is None else stats
    vx = _view(d["x"], xcoff, cin, d.get("xtab"), d.get("xgate"))
    y = torch.full((n, ho, wo, ycs), PREFILL, device=dev)
    vy = _view(y, ycoff, cout)
    sbuf = torch.zeros(32, 2, cout, dtype=torch.float64, device=dev) if with_stats else None
    scr = _scratch(c, dev, wt)
    rc = L.lhn_conv_kxk_fwd(C.byref(vx), _lib.ptr(d["w"]), C.byref(vy), _lib.ptr(sbuf), stride, None, _lib.ptr(scr), st)
    torch.cuda.synchronize()
    if expect_fail:
        return rc, {"y": bool((y == PREFILL).all()), "wt_scratch": bool((scr == PREFILL).all()),
                    "stats": sbuf is None or bool((sbuf == 0).all())}
    _lib.check(rc, f"kxk fwd {name}")
    out = {"y": y[..., ycoff:ycoff + cout].cpu().numpy(),
           "y_outside_ok": np.array(bool((_outside(y, ycoff, cout) == PREFILL).all()))}
    if sbuf is not None:
        tot = sbuf.sum(0).cpu().numpy()
        out["stats_sum"], out["stats_sq"] = tot[0], tot[1]        # two outputs: each row against its own scale
    if scr is not None:
        out["wt_ok"] = np.array(torch.equal(scr[:-SLACK].view(9, cout, cin), d["w"].view(cout, cin, 9).permute(2, 0, 1)) and
                                bool((scr[-SLACK:] == PREFILL).all()))
    return out


def run_bwd(name, dev, g=None, wt=True, expect_fail=False):
    """Outputs of lhn_conv_kxk_bwd: dx (the view's channels), dW (replicas summed, [Cout][Cin][3][3]), dz of the view after the
    call where the plain path ran (k_dy_inplace: dz := dy); `*_ok` flags: floats that must keep their bits did."""
    c = _ALL["bwd"][name]
    f, (n, h, w), cin, cout, stride = c["flags"], c["nhw"], c["cin"], c["cout"], c["stride"]
    xcs, xcoff, ycs, ycoff, ho, wo = geometry("bwd", name)
    g = g or inputs("bwd", name)
    d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in g.items()}
    L, st = _lib.lib(), _lib.stream()
    vx = _view(d["x"], xcoff, cin, d["xtab"], d.get("xgate"))
    vy = _view(d["y"], ycoff, cout, d["ytab"], d.get("ygate"))
    dz = d["dz"].clone()                             # a fresh clone per call: the plain path consumes it
    gv = GradView()
    gv.dz, gv.dpool, gv.coef = dz.data_ptr(), (d["dpool"].data_ptr() if "dpool" in d else None), d["coef"].data_ptr()
    nrep = _nrep(c)
    nw = cout * cin * 9
    rs = nw + SLACK                                  # one replica: dW | slack
    gbuf = torch.zeros(nrep, rs, device=dev)
    if "nodx" in f:
        dx, acc = None, 0
    elif "prior" in d:
        dx, acc = d["prior"].clone(), 1
    else:
        dx, acc = torch.full((n, h, w, xcs), PREFILL, device=dev), 0
    scr = _scratch(c, dev, wt)
    rc = L.lhn_conv_kxk_bwd(C.byref(vx), _lib.ptr(d["w"]), C.byref(vy), C.byref(gv), _lib.ptr(dx), acc, _lib.ptr(gbuf), stride, nrep,
                            C.c_int64(rs), _lib.ptr(scr), st)
    torch.cuda.synchronize()
    if expect_fail:
        return rc, {"dw": bool((gbuf == 0).all()), "dz": torch.equal(dz, d["dz"]), "dx": bool((dx == PREFILL).all()),
                    "wt_scratch": bool((scr == PREFILL).all())}
    _lib.check(rc, f"kxk bwd {name}")
    out = {"dw": gbuf.sum(0)[:nw].view(cout, cin, 3, 3).cpu().numpy(),
           "dw_pad_ok": np.array(bool((gbuf[:, nw:] == 0).all()))}           # every replica's slack
    if dx is not None:
        out["dx"] = dx[..., xcoff:xcoff + cin].cpu().numpy()
        before = d["prior"] if "prior" in d else torch.full_like(dx, PREFILL)
        out["dx_outside_ok"] = np.array(torch.equal(_outside(dx, xcoff, cin), _outside(before, xcoff, cin)))
    if plain_path(c):
        out["dz"] = dz[..., ycoff:ycoff + cout].cpu().numpy()
        out["dz_outside_ok"] = np.array(torch.equal(_outside(dz, ycoff, cout), _outside(d["dz"], ycoff, cout)))
    else:
        out["dz_unchanged_ok"] = np.array(torch.equal(dz, d["dz"]))          # dy on the fly: dz is only read
    if scr is not None:
        ok = bool((scr[-SLACK:] == PREFILL).all())
        if dx is None:
            ok = ok and bool((scr == PREFILL).all())                         # no dgrad: the scratch is not used
        else:                                                                # dgrad layout: wt[tap][ci][co] = w[co][ci][tap]
            ok = ok and torch.equal(scr[:-SLACK].view(9, cin, cout), d["w"].view(cout, cin, 9).permute(2, 1, 0))
        out["wt_ok"] = np.array(ok)
    return out


# ---------------------------------------------------------------- references
def reference_fwd(name, g=None, dtype=torch.float64, stats=None):
    c = _ALL["fwd"][name]
    f, cin, cout, s = c["flags"], c["cin"], c["cout"], c["stride"]
    xcs, xcoff, ycs, ycoff, ho, wo = geometry("fwd", name)
    g = g or inputs("fwd", name)
    sl = slice(xcoff, xcoff + cin)
    cut = lambda t: (t[..., sl] if t is not None else None)  # noqa: E731
    X = _value(g["x"][..., sl], cut(g.get("xtab")), cut(g.get("xgate")), dtype)
    y = F.conv2d(X.permute(0, 3, 1, 2), g["w"].to(dtype), stride=s, padding=1).permute(0, 2, 3, 1)
    out = {"y": y.double().numpy()}
    if ("nostats" not in f) if stats is None else stats:
        out["stats_sum"], out["stats_sq"] = y.sum((0, 1, 2)).double().numpy(), (y * y).sum((0, 1, 2)).double().numpy()
    return out


def reference_bwd(name, g=None, dtype=torch.float64):
    """dx, dw and `dz`: the dy that the view's channels of dz hold after a call on the plain path."""
    c = _ALL["bwd"][name]
    f, (n, h, w), cin, cout, s = c["flags"], c["nhw"], c["cin"], c["cout"], c["stride"]
    xcs, xcoff, ycs, ycoff, ho, wo = geometry("bwd", name)
    g = g or inputs("bwd", name)
    xs, ys = slice(xcoff, xcoff + cin), slice(ycoff, ycoff + cout)
    X = _value(g["x"][..., xs], g["xtab"][:, xs], g["xgate"][:, xs] if "xgate" in g else None, dtype)
    wt = g["w"].to(dtype)
    e = g["dz"][..., ys].to(dtype)
    if "ygate" in g:
        e = e * g["ygate"][:, ys].to(dtype)[:, None, None, :]
    if "dpool" in g:
        slot = torch.tensor([[_seg(i, ho) * 5 + _seg(j, wo) for j in range(wo)] for i in range(ho)])
        e = e + g["dpool"][:, :, ys].to(dtype)[:, slot.view(-1)].view(n, ho, wo, cout)
    du = e * _dact(g["y"][..., ys], g["ytab"][:, ys], dtype)
    A, B, Cc = (g["coef"][i, ys].to(dtype) for i in range(3))
    dy = A * du + B * g["y"][..., ys].to(dtype) + Cc
    out = {"dz": dy.double().numpy()}
    dyn, Xn = dy.permute(0, 3, 1, 2).contiguous(), X.permute(0, 3, 1, 2).contiguous()
    out["dw"] = torch.nn.grad.conv2d_weight(Xn, wt.shape, dyn, stride=s, padding=1).double().numpy()
    if "nodx" not in f:
        dxv = torch.nn.grad.conv2d_input(Xn.shape, wt, dyn, stride=s, padding=1).permute(0, 2, 3, 1)
        out["dx"] = (dxv + g["prior"][..., xs].to(dtype) if "prior" in g else dxv).double().numpy()
    return out


def run(kind, name, dev, g=None):
    return run_fwd(name, dev, g) if kind == "fwd" else run_bwd(name, dev, g)


def reference(kind, name, g=None, dtype=torch.float64):
    return reference_fwd(name, g, dtype) if kind == "fwd" else reference_bwd(name, g, dtype)


def _check_reference():
    import time
    t0, worst = time.time(), 0.0
    for kind, tab in TABLES.items():
        for nm in tab:
            g = inputs(kind, nm)
            assert g["seed"] == 7, f"{kind}:{nm} needed seed {g['seed']}"
            r64, r32 = reference(kind, nm, g), reference(kind, nm, g, torch.float32)
            for k in r64:
                assert np.isfinite(r64[k]).all(), f"{kind}:{nm} {k}"
                worst = max(worst, rel_err(r32[k], r64[k]))
    print(f"{sum(len(t) for t in TABLES.values())} cases, no activation kinks at seed 7, worst float32 error {worst:.2e}, {time.time() - t0:.1f} s")


def _instances():
    """profiles/kxk_instances.md: one table per direction and setting; under a switch only the cases that change their launches."""
    import kxk256_cases  # noqa: F401  (registers its tables in _ALL)
    tables = {k: list(TABLES[k]) + list(kxk256_cases.TABLES[k]) for k in TABLES}
    print("# Dense 3x3 convolution kernels: which test case launches what\n")
    print("The answers of `lhn_conv_kxk_route` (`include/lhn.h`: host only, the route functions `lhn_conv_kxk_fwd` / `lhn_conv_kxk_bwd` ask) for\n"
          "`FWD` / `BWD` of `tests/kxk_cases.py` and `tests/kxk256_cases.py`, printed by `python tests/kxk_cases.py --instances`;\n"
          "`tests/test_kxk_route_cpu.py` holds them as a literal table.  `k_kxk<KD, NT, MODE, TAPS, PLAIN>` (MODE 0 forward, 1 data gradient),\n"
          "`k_kxk_wgrad<CIN, NTO, TAPS, PLAIN>`: names as a kernel trace prints them, launches in order, every case with the tap-major weight\n"
          "scratch (`k_w_tapmajor`).  Behind a name: ` yN` N blocks of features on `gridDim.y`, ` par` the four pixel-parity classes of the\n"
          "stride-2 data gradient, ` zN` N groups of output channels on `gridDim.z`, ` excl` / ` atomic` the weight gradient's flush, ` x 2` one\n"
          "launch per 128-channel input slice.")
    for kind, title in (("fwd", "Forward"), ("bwd", "Backward")):
        base = {nm: kernel_of(kind, nm) for nm in tables[kind]}
        for setting, kw in SETTINGS:
            got = {nm: kernel_of(kind, nm, **kw) for nm in tables[kind]}
            rows = {}
            for nm, k in got.items():
                if not kw or k != base[nm]:
                    rows.setdefault(k, []).append(nm)
            if not rows:
                continue
            print(f"\n## {title}, {setting}" + (": the cases that change their launches" if kw else "") + "\n\n| launches | cases |\n|---|---|")
            for k, names in rows.items():
                print(f"| `{k}` | {', '.join(names)} |")
    print("\n## Refused for lack of a kernel (the query answers NULL)\n")
    print(", ".join(f"{kind}:{nm}" for kind in ("fwd", "bwd") for nm in _ALL[kind] if nm not in tables[kind] and kernel_of(kind, nm) is None))


if __name__ == "__main__":
    if sys.argv[1] == "--instances":
        import kxk_cases          # (kxk256_cases registers its tables in the imported module, not in __main__)
        kxk_cases._instances()
        sys.exit(0)
    if sys.argv[1] == "--check-reference":
        _check_reference()
        sys.exit(0)
    dst, reps, names = sys.argv[1], int(sys.argv[2]), sys.argv[3:]
    dev = torch.device("cuda:0")
    res = {}
    for full in names:
        kind, nm = full.split(":")
        g = inputs(kind, nm)
        for r in range(reps):
            for k, v in run(kind, nm, dev, g).items():
                res[f"{full}/{r}/{k}"] = v
    np.savez(dst, **res)
