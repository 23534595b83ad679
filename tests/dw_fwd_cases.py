"""Cases of the depthwise forward (lhn_conv_dw_fwd / _fwd2 / _fwd3, csrc/k_conv_dw.hip) run through the C ABI, with a plain torch
reference on the CPU (float64, or float32 to measure what the same operation loses in the kernels' own precision).  Imported by
tests/test_dw_fwd_gpu.py; run as a script (a child process with its own environment: LHN_DW_GATHER=1, LHN_XCD_ORDER=1 or
LHN_DETERMINISTIC=1) it writes the kernel outputs of the named cases to an .npz file:
    python tests/dw_fwd_cases.py OUT.npz REPEATS NAME ...
    python tests/dw_fwd_cases.py --check-reference        (CPU only: every case's inputs, both references, the dispatch table)

kernel_of(name) asks the library which kernel a case runs (lhn_conv_dw_route); profiles/dw_instances.md is printed from it."""
import ctypes as C
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pw_cases import PREFILL, _lib, _outside, _rand, _view, rel_err  # noqa: E402,F401
from litehandnet_amd._lib import View  # noqa: E402

STAT_REPLICAS = 32              # LHN_STAT_REPLICAS (include/lhn.h)
TICKET_WORDS = 33               # lhn_bnfin.counter: one top word + 32 group words
STAT_PAD = 64                   # doubles behind the statistics: must stay zero (a channel tail that counted a dead lane lands here)
COEF2 = (0.7, -1.3)
EPS, MOMENTUM, SLOPE = 1e-5, 0.1, 0.1


class BnFin(C.Structure):        # lhn_bnfin (include/lhn.h)
    _fields_ = [("counter", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("running_mean", C.c_void_p),
                ("running_var", C.c_void_p), ("num_batches_tracked", C.c_void_p), ("table", C.c_void_p), ("save_mean_invstd", C.c_void_p),
                ("count", C.c_double), ("cstride", C.c_int32), ("coff", C.c_int32), ("C", C.c_int32),
                ("eps", C.c_float), ("momentum", C.c_float), ("slope", C.c_float), ("conv_bias", C.c_void_p)]


def _case(n, h, w, c, k=3, s=1, d=1, p=None, flags="", xv=None, yv=None, **kw):
    """x is channels [xcoff, xcoff + c) of a buffer of xcs channels (default: [4, 4 + c) of c + 12), y likewise ([8, 8 + c) of c + 8)."""
    xcs, xcoff = xv or (c + 12, 4)
    ycs, ycoff = yv or (c + 8, 8)
    return dict(n=n, h=h, w=w, c=c, k=k, s=s, d=d, p=(d * (k - 1) // 2 if p is None else p), flags=flags.split(), xcs=xcs, xcoff=xcoff,
                ycs=ycs, ycoff=ycoff, **kw)


# flags: gate: per-(n, c) gate on x;  notab: no pending transform on x;  extra: a second source (own buffer, table and gate),
# through lhn_conv_dw_fwd3;  sumout: ... with sum_out into a slice of a wider buffer;  fwd2: ... through lhn_conv_dw_fwd2;
# wnull: w = NULL (k = 1 identity);  fin: fused BatchNorm finalize;  bias: ... with a conv_bias
CASES = {}
# 1. k_dwk_fwd_lds<3,1>: tile 8 x 32 pixels, 32 channels per group
CASES["lds3_16"] = _case(2, 16, 16, 64)
CASES["lds3_9x37"] = _case(1, 9, 37, 32)                                   # ragged both ways, two column tiles
CASES["lds3_8"] = _case(2, 8, 8, 32)                                       # W = 8: the narrowest tiled map
CASES["lds3_16x33_gate"] = _case(3, 16, 33, 64, flags="gate")
CASES["lds3_c20"] = _case(2, 11, 13, 20, xv=(40, 8), yv=(32, 4))           # five valid lanes
CASES["lds3_c40"] = _case(2, 11, 13, 40)                                   # second group: two lanes
CASES["lds3_c80"] = _case(1, 11, 13, 80)
CASES["lds3_notab"] = _case(4, 16, 32, 32, flags="notab")                  # 8 tiles: a multiple of 8 * cgroups (LHN_XCD_ORDER)
# 2. dilation 2, W >= 16: four parity sub-lattices on <3,1>, ps = 2
CASES["par_32"] = _case(2, 32, 32, 64, d=2)
CASES["par_17x19"] = _case(2, 17, 19, 32, d=2)                             # the four sub-lattices differ in extent
CASES["par_3x16"] = _case(1, 3, 16, 32, d=2)                               # odd rows: a sub-lattice of one row
CASES["par_16_c40_gate"] = _case(2, 16, 16, 40, d=2, flags="gate")
# 3. k_dwk_fwd_lds<3,2>: dilation 2, 8 <= W < 16
CASES["d2_8"] = _case(3, 8, 8, 64, d=2)
CASES["d2_12x13_c20"] = _case(2, 12, 13, 20, d=2)
# 4. k_dwk_fwd_lds<7,1>
CASES["k7_16"] = _case(2, 16, 16, 32, k=7)
CASES["k7_9x11_c40_gate"] = _case(1, 9, 11, 40, k=7, flags="gate")
# 5. two sources, <3,1,2>
CASES["ex_16_so"] = _case(2, 16, 16, 64, flags="gate extra sumout")
CASES["ex_16"] = _case(2, 16, 16, 64, flags="gate extra")
CASES["ex_16_fwd2"] = _case(2, 16, 16, 64, flags="gate extra fwd2")
CASES["ex_9x37_c20_so"] = _case(1, 9, 37, 20, flags="gate extra sumout")
CASES["ex_9x37_c20"] = _case(1, 9, 37, 20, flags="gate extra")
CASES["ex_par_17x19_so"] = _case(2, 17, 19, 32, d=2, flags="gate extra sumout")
CASES["ex_par_17x19"] = _case(2, 17, 19, 32, d=2, flags="gate extra")
# 6. k_dws2_fwd_lds: 3x3, stride 2, pad 1 (tile 4 x 16 outputs)
CASES["s2_16"] = _case(2, 16, 16, 64, s=2)
CASES["s2_17x19"] = _case(2, 17, 19, 32, s=2)
CASES["s2_9_c20_gate"] = _case(1, 9, 9, 20, s=2, flags="gate")
CASES["s2_34x66"] = _case(2, 34, 66, 32, s=2)                              # 17 x 33 outputs: more than one tile each way
# 7. the row-gather kernel k_dw_fwd<K>, reached by shape
CASES["g3_4x4"] = _case(2, 4, 4, 64)                                       # C4 = 16: the shuffle reduction
CASES["g3_2x2"] = _case(2, 2, 2, 64)
CASES["g3_1x1"] = _case(3, 1, 1, 64)
CASES["g3_7x5_c128"] = _case(2, 7, 5, 128)
CASES["g1_w"] = _case(2, 9, 9, 32, k=1)
CASES["g1_identity"] = _case(2, 6, 10, 64, k=1, flags="gate wnull")
CASES["g5_9"] = _case(2, 9, 9, 32, k=5)
CASES["g7_6x6"] = _case(2, 6, 6, 32, k=7)
CASES["g3_valid"] = _case(2, 10, 10, 32, p=0)                              # the 'valid' 3x3 of common.py
CASES["g3_s2d2"] = _case(2, 11, 13, 32, s=2, d=2)
CASES["g3_c256"] = _case(1, 4, 4, 256)                                     # C4 = 64 > 32: the LDS reduction
CASES["g3_c512"] = _case(1, 3, 5, 512)
CASES["g3_c20"] = _case(2, 5, 7, 20, xv=(40, 8), yv=(32, 4))               # C4 = 5: 51 pixel lanes, thread 255 is dead
CASES["g3_c40"] = _case(2, 5, 7, 40)                                       # C4 = 10: 25 pixel lanes, threads 250.. are dead
# 8. fused BatchNorm finalize
CASES["fin_lds3"] = _case(2, 16, 16, 64, flags="fin")
CASES["fin_s2_bias"] = _case(2, 17, 19, 32, s=2, flags="fin bias")
CASES["fin_g3_4x4"] = _case(2, 4, 4, 64, flags="gate fin")

NOSTATS_TWICE = ["lds3_9x37", "par_17x19", "s2_17x19", "g3_c20", "ex_9x37_c20_so"]

# calls the library must refuse (non-zero status, the reason in lhn_last_error, nothing written)
REFUSE = {
    "c6": _case(2, 8, 8, 6, xv=(8, 0), yv=(8, 0), refuse="bad view"),
    "c516": _case(1, 4, 4, 516, refuse="channels 516"),
    "k2": _case(2, 8, 8, 32, k=2, p=0, refuse="k=2"),
    "wrong_out": _case(2, 8, 8, 32, flags="badout", refuse="expected 8x8"),
    "sum_out_alone": _case(2, 8, 8, 32, flags="sumonly", refuse="sum_out without a second source"),
    "extra_k7": _case(2, 16, 16, 32, k=7, flags="extra sumout", refuse="a second source needs k=3"),
    "extra_s2": _case(2, 16, 16, 32, s=2, flags="extra sumout", refuse="same-size output"),
    "extra_w4": _case(2, 4, 4, 32, flags="extra sumout", refuse="a second source needs k=3"),
    "extra_d2_w12": _case(2, 12, 12, 32, d=2, flags="extra sumout", refuse="a second source needs k=3"),
    "sum_out_misaligned": _case(2, 8, 8, 32, flags="extra sumout somis", refuse="sum_out geometry"),
}
_ALL = dict(CASES, **REFUSE)


def out_hw(c):
    f = lambda e: (e + 2 * c["p"] - c["d"] * (c["k"] - 1) - 1) // c["s"] + 1      # noqa: E731
    return f(c["h"]), f(c["w"])


def kernel_of(name, gather=False):
    """The kernel lhn_conv_dw_fwd / lhn_conv_dw_fwd3 launch for a case, asked of the library (lhn_conv_dw_route: host only).
    gather: under LHN_DW_GATHER=1.  None: no kernel for the case."""
    c = _ALL[name]
    feat = 1 * ("wnull" in c["flags"]) | 2 * ("extra" in c["flags"])        # LHN_DW_F_NO_WEIGHT, LHN_DW_F_EXTRA (include/lhn.h)
    r = _lib.lib().lhn_conv_dw_route(0, c["h"], c["w"], c["c"], c["k"], c["s"], c["p"], c["d"], feat, 1 if gather else 0)   # LHN_DW_SW_GATHER
    return r.decode() if r is not None else None


def xcd_grid(name, cus=256):
    """(grid, xchunk) of a tiled stride-1 case as launch_dwk_fwd / dw3_grid / dw3_xchunk compute them under LHN_XCD_ORDER=1."""
    c = _ALL[name]
    ps = 2 if (c["d"] == 2 and c["w"] >= 16) else 1
    cg = (c["c"] + 31) // 32
    sh, sw = (c["h"] + ps - 1) // ps, (c["w"] + ps - 1) // ps
    ntile = c["n"] * ps * ps * ((sh + 7) // 8) * ((sw + 31) // 32) * cg
    g = cus * 2                      # the smallest cap of launch_dwk_fwd (one block per CU by LDS, times 2)
    g -= g % cg
    g = max(min(g, ntile), cg)
    return g, (g // 8 if g % (8 * cg) == 0 else 0)


def _tab(cs, seed):
    """scale | shift | slope 0.1; every third channel has a negative scale"""
    sign = torch.where(torch.arange(cs) % 3 == 1, -1.0, 1.0)
    return torch.stack([sign * (1 + 0.3 * _rand((cs,), seed)), 0.2 * _rand((cs,), seed + 1), torch.full((cs,), 0.1)]).contiguous()


def inputs(name, seed=7):
    c = _ALL[name]
    f, n, h, w, ch, k = c["flags"], c["n"], c["h"], c["w"], c["c"], c["k"]
    g = {"seed": seed}
    g["x"] = _rand((n, h, w, c["xcs"]), seed)
    if "wnull" not in f:
        g["w"] = _rand((ch, k * k), seed + 3, 1.5 / k)
    if "notab" not in f:
        g["xtab"] = _tab(c["xcs"], seed + 4)
    if "gate" in f:
        g["xgate"] = torch.sigmoid(_rand((n, c["xcs"]), seed + 11))
    if "extra" in f:
        ecs = ch + 20
        g["e"] = _rand((n, h, w, ecs), seed + 30)
        g["etab"] = _tab(ecs, seed + 40)
        g["egate"] = torch.sigmoid(_rand((n, ecs), seed + 50))
    if "fin" in f:
        g["gamma"], g["beta"] = 1 + 0.2 * _rand((ch,), seed + 60), 0.3 * _rand((ch,), seed + 61)
        g["rmean"], g["rvar"] = 0.1 * _rand((ch,), seed + 62), 1 + 0.2 * _rand((ch,), seed + 63).abs()
        if "bias" in f:
            g["cbias"] = 0.5 * _rand((ch,), seed + 64)
    return g


ECOFF, SOCOFF = 12, 8            # channel offsets of the second source (buffer of c + 20) and of sum_out (buffer of c + 16)


# ---------------------------------------------------------------- kernels
def run(name, dev, g=None, stats=True, expect_fail=False, fin_separate=True):
    """Outputs of the forward as numpy arrays (the view's channels), plus `*_ok` flags: every float outside the outputs still
    holds its prefill, bit for bit.  A `fin` case also runs lhn_bn_finalize as a launch of its own on the statistics the call left
    behind and reports whether the two tables agree in every bit (`sep_bits_equal`)."""
    c = _ALL[name]
    f, n, h, w, ch, k = c["flags"], c["n"], c["h"], c["w"], c["c"], c["k"]
    xcs, xcoff, ycs, ycoff = c["xcs"], c["xcoff"], c["ycs"], c["ycoff"]
    ho, wo = out_hw(c)
    if "badout" in f:
        ho += 1
    g = g or inputs(name)
    d = {kk: (v.to(dev) if torch.is_tensor(v) else v) for kk, v in g.items()}
    L, st = _lib.lib(), _lib.stream()
    vx = _view(d["x"], xcoff, ch, d.get("xtab"), d.get("xgate"))
    y = torch.full((n, ho, wo, ycs), PREFILL, device=dev)
    vy = _view(y, ycoff, ch)
    sbuf = torch.zeros(STAT_REPLICAS * 2 * ch + STAT_PAD, dtype=torch.float64, device=dev) if stats else None
    ev = so = sv = None
    if "extra" in f:
        ev = _view(d["e"], ECOFF, ch, d["etab"], d["egate"])
    if "sumout" in f or "sumonly" in f:
        so = torch.full((n, h, w, ch + 16), PREFILL, device=dev)
        sv = _view(so, SOCOFF, ch)
        if "somis" in f:
            sv.coff = SOCOFF + 2
    fin, fb = None, {}
    if "fin" in f:
        fb = {"counter": torch.zeros(TICKET_WORDS, dtype=torch.int32, device=dev), "table": torch.full((3, ycs), PREFILL, device=dev),
              "save": torch.full((2, ch), PREFILL, device=dev), "rmean": d["rmean"].clone(), "rvar": d["rvar"].clone(),
              "nbt": torch.full((1,), 5, dtype=torch.int64, device=dev)}
        fin = BnFin()
        fin.counter, fin.gamma, fin.beta = fb["counter"].data_ptr(), d["gamma"].data_ptr(), d["beta"].data_ptr()
        fin.running_mean, fin.running_var, fin.num_batches_tracked = fb["rmean"].data_ptr(), fb["rvar"].data_ptr(), fb["nbt"].data_ptr()
        fin.table, fin.save_mean_invstd, fin.count = fb["table"].data_ptr(), fb["save"].data_ptr(), float(n * ho * wo)
        fin.cstride, fin.coff, fin.C, fin.eps, fin.momentum, fin.slope = ycs, ycoff, ch, EPS, MOMENTUM, SLOPE
        fin.conv_bias = d["cbias"].data_ptr() if "cbias" in d else None
    finp = C.byref(fin) if fin is not None else None
    coef2 = (C.c_float * 2)(*COEF2)
    wp = _lib.ptr(d.get("w"))
    geo = (k, c["s"], c["p"], c["d"])
    if "fwd2" in f:
        rc = L.lhn_conv_dw_fwd2(C.byref(vx), wp, C.byref(vy), _lib.ptr(sbuf), *geo, finp, C.byref(ev), coef2, st)
    elif ev is not None or sv is not None:
        rc = L.lhn_conv_dw_fwd3(C.byref(vx), wp, C.byref(vy), _lib.ptr(sbuf), *geo, finp, C.byref(ev) if ev is not None else None, coef2,
                                C.byref(sv) if sv is not None else None, st)
    else:
        rc = L.lhn_conv_dw_fwd(C.byref(vx), wp, C.byref(vy), _lib.ptr(sbuf), *geo, finp, st)
    torch.cuda.synchronize()
    if expect_fail:
        return rc, bool((y == PREFILL).all()) and (so is None or bool((so == PREFILL).all())) and (sbuf is None or bool((sbuf == 0).all()))
    _lib.check(rc, f"dw fwd {name}")
    out = {"y": y[..., ycoff:ycoff + ch].cpu().numpy(), "y_outside_ok": np.array(bool((_outside(y, ycoff, ch) == PREFILL).all()))}
    if sbuf is not None:
        tot = sbuf[:STAT_REPLICAS * 2 * ch].view(STAT_REPLICAS, 2, ch).sum(0).cpu().numpy()
        out["stats_sum"], out["stats_sq"] = tot[0], tot[1]        # two outputs: each row against its own scale
        out["stats_pad_ok"] = np.array(bool((sbuf[STAT_REPLICAS * 2 * ch:] == 0).all()))
    if so is not None:
        out["sum_out"] = so[..., SOCOFF:SOCOFF + ch].cpu().numpy()
        out["sum_outside_ok"] = np.array(bool((_outside(so, SOCOFF, ch) == PREFILL).all()))
    if fin is not None:
        tab = fb["table"][:, ycoff:ycoff + ch].cpu().numpy()
        out["fin_scale"], out["fin_shift"], out["fin_slope"] = tab[0], tab[1], tab[2]
        out["fin_mean"], out["fin_invstd"] = fb["save"][0].cpu().numpy(), fb["save"][1].cpu().numpy()
        out["fin_rmean"], out["fin_rvar"] = fb["rmean"].cpu().numpy(), fb["rvar"].cpu().numpy()
        out["fin_nbt"] = fb["nbt"].cpu().numpy()
        out["table_outside_ok"] = np.array(bool((_outside(fb["table"], ycoff, ch) == PREFILL).all()))
        if fin_separate:
            t2, s2 = torch.full((3, ycs), PREFILL, device=dev), torch.full((2, ch), PREFILL, device=dev)
            rm2, rv2, nbt2 = d["rmean"].clone(), d["rvar"].clone(), torch.full((1,), 5, dtype=torch.int64, device=dev)
            _lib.check(L.lhn_bn_finalize(_lib.ptr(sbuf), _lib.ptr(d["gamma"]), _lib.ptr(d["beta"]), _lib.ptr(rm2), _lib.ptr(rv2), _lib.ptr(nbt2),
                                         _lib.ptr(t2), ycs, ycoff, ch, _lib.ptr(s2), C.c_double(n * ho * wo), C.c_float(EPS),
                                         C.c_float(MOMENTUM), C.c_float(SLOPE), 1, _lib.ptr(d.get("cbias")), st), "bn finalize")
            torch.cuda.synchronize()
            same = all(torch.equal(a, b) for a, b in ((t2, fb["table"]), (s2, fb["save"]), (rm2, fb["rmean"]), (rv2, fb["rvar"]), (nbt2, fb["nbt"])))
            out["sep_bits_equal"] = np.array(same)
            out["sep_scale"], out["sep_shift"] = t2[0, ycoff:ycoff + ch].cpu().numpy(), t2[1, ycoff:ycoff + ch].cpu().numpy()
            out["sep_rmean"], out["sep_rvar"] = rm2.cpu().numpy(), rv2.cpu().numpy()
    return out


# ---------------------------------------------------------------- reference
def _value(raw, tab, gate, dt):
    v = raw.to(dt)
    if tab is not None:
        u = v * tab[0].to(dt) + tab[1].to(dt)
        v = torch.where(u > 0, u, u * tab[2].to(dt))
    if gate is not None:
        v = v * gate.to(dt)[:, None, None, :]
    return v


def reference(name, g=None, dtype=torch.float64, stats=True):
    """value(x) [+ value(extra)] -> conv2d(groups = C) over ZERO padding of the value; the statistics and the BatchNorm of y."""
    c = _ALL[name]
    f, n, ch, k = c["flags"], c["n"], c["c"], c["k"]
    g = g or inputs(name)
    xs = slice(c["xcoff"], c["xcoff"] + ch)
    cut = lambda t, sl: (t[..., sl] if t is not None else None)      # noqa: E731
    X = _value(g["x"][..., xs], cut(g.get("xtab"), xs), cut(g.get("xgate"), xs), dtype)
    out = {}
    if "extra" in f:
        es = slice(ECOFF, ECOFF + ch)
        X = COEF2[0] * X + COEF2[1] * _value(g["e"][..., es], g["etab"][..., es], g["egate"][..., es], dtype)
        if "sumout" in f:
            out["sum_out"] = X.double().numpy()
    wt = g["w"].to(dtype).view(ch, 1, k, k) if "w" in g else torch.ones(ch, 1, 1, 1, dtype=dtype)
    y = F.conv2d(X.permute(0, 3, 1, 2), wt, None, c["s"], c["p"], c["d"], ch).permute(0, 2, 3, 1)
    out["y"] = y.double().numpy()
    if stats:
        out["stats_sum"], out["stats_sq"] = y.sum((0, 1, 2)).double().numpy(), (y * y).sum((0, 1, 2)).double().numpy()
    if "fin" in f:
        cnt = y.numel() // ch
        mean, var = y.mean((0, 1, 2)), y.var((0, 1, 2), unbiased=False)
        invstd = 1.0 / torch.sqrt(var + EPS)
        scale = g["gamma"].to(dtype) * invstd
        cb = g["cbias"].to(dtype) if "cbias" in g else 0.0
        out["fin_scale"], out["fin_shift"] = scale.double().numpy(), (g["beta"].to(dtype) - mean * scale).double().numpy()
        out["fin_slope"] = np.full(ch, np.float32(SLOPE), np.float64)
        out["fin_mean"], out["fin_invstd"] = mean.double().numpy(), invstd.double().numpy()
        out["fin_rmean"] = ((1 - MOMENTUM) * g["rmean"].to(dtype) + MOMENTUM * (mean + cb)).double().numpy()
        out["fin_rvar"] = ((1 - MOMENTUM) * g["rvar"].to(dtype) + MOMENTUM * var * cnt / (cnt - 1)).double().numpy()
    return out


def _check_reference():
    import time
    t0, worst = time.time(), 0.0
    for nm in CASES:
        g = inputs(nm)
        r64, r32 = reference(nm, g), reference(nm, g, torch.float32)
        for k in r64:
            assert np.isfinite(r64[k]).all() and np.abs(r64[k]).max() > 0, f"{nm} {k}: reference not finite or all zeros"
            e = rel_err(r32[k], r64[k])
            assert np.isfinite(3 * e), f"{nm} {k}"
            worst = max(worst, e)
        print(f"{nm:22s} {kernel_of(nm):28s} gather: {kernel_of(nm, True)}")
    print(f"{len(CASES)} cases, worst float32 error {worst:.2e}, {time.time() - t0:.1f} s")


if __name__ == "__main__":
    if sys.argv[1] == "--check-reference":
        _check_reference()
        sys.exit(0)
    dst, reps, names = sys.argv[1], int(sys.argv[2]), sys.argv[3:]
    dev = torch.device("cuda:0")
    res = {}
    for nm in names:
        g = inputs(nm)
        for r in range(reps):
            for k, v in run(nm, dev, g).items():
                res[f"{nm}/{r}/{k}"] = v
    np.savez(dst, **res)
