"""Cases of the stem convolution (lhn_conv_stem_fwd / lhn_conv_stem_bwd, csrc/k_conv_stem.hip: dense k x k on the 3-channel NCHW image)
run through the C ABI, with a plain torch reference on the CPU (float64, or float32 to measure what the same operation loses in
the kernels' own precision).  Imported by tests/test_stem_gpu.py; run as a script (a child process with its own environment:
LHN_DW_GATHER=1 or LHN_DETERMINISTIC=1) it writes the kernel outputs of the named cases to an .npz file:
    python tests/stem_cases.py OUT.npz REPEATS fwd:NAME bwd:NAME ...
    python tests/stem_cases.py --check-reference        (CPU only: every case's inputs, both references, the dispatch table)

kernel_of(name, gather, kind) repeats the dispatch of lhn_conv_stem_fwd / lhn_conv_stem_bwd."""
import ctypes as C
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pw_cases import PREFILL, _dact, _kinks, _lib, _nrep, _outside, _rand, _seg, _tab, _view, rel_err  # noqa: E402,F401
from dw_fwd_cases import STAT_PAD, STAT_REPLICAS, TICKET_WORDS, BnFin  # noqa: E402
from litehandnet_amd._lib import GradView  # noqa: E402

EPS, MOMENTUM, SLOPE = 1e-5, 0.1, 0.1
DW_SLACK = 16                    # floats behind each gradient replica: must keep their prefill
DIRECT_LDS_LIMIT = 65536         # bytes of dynamic LDS the direct forward kernel may ask for (include/lhn.h)


def _case(n, hi, wi, k, s, p, cout, flags="", yv=None, **kw):
    """y is channels [ycoff, ycoff + cout) of a buffer of ycs channels (default: [8, 8 + cout) of cout + 8)."""
    ycs, ycoff = yv or (cout + 8, 8)
    return dict(n=n, hi=hi, wi=wi, k=k, s=s, p=p, cout=cout, flags=flags.split(), ycs=ycs, ycoff=ycoff, **kw)


# forward flags: fin: fused BatchNorm finalize;  bias: ... with a conv_bias;  offset: the large-mean image and weights
# backward flags (every case has a y table, a coef table and _nrep(c) gradient replicas with a prior): ygate / dpool: gate and
# pooled gradient on y;  nocoef: coef = NULL (dy = du);  notab: y without a table;  fold: replicas folded by lhn_reduce_replicas
CASES = {}
# 1. k_stem3_fwd_mfma / k_stem3_bwd_mfma: 3x3 -> 32, tiles of 256 pixels
CASES["m3_32"] = _case(2, 32, 32, 3, 2, 1, 32, "fold")                      # two full tiles
CASES["m3_33x29"] = _case(2, 33, 29, 3, 2, 1, 32, "fin ygate dpool")        # 17 x 15 outputs, 510 px: tile 0 straddles the images, 2 dead pixels
CASES["m3_tiny"] = _case(1, 5, 7, 3, 2, 1, 32, "nocoef")                    # 12 px: three waves entirely dead (cnt == 0)
CASES["m3_s1"] = _case(1, 9, 13, 3, 1, 1, 32)                               # stride 1 through the same kernel
CASES["m3_valid"] = _case(1, 11, 11, 3, 2, 0, 32)                           # no padding
CASES["m3_whole"] = _case(2, 16, 16, 3, 2, 1, 32, yv=(32, 0))               # y is the whole buffer
# 2. k_stem7_fwd_mfma / k_stem7_bwd_mfma: 7x7 -> 64, tiles of 64 pixels
CASES["m7_32"] = _case(2, 32, 32, 7, 2, 3, 64)                              # eight full tiles
CASES["m7_23x19"] = _case(2, 23, 19, 7, 2, 3, 64, "fin bias ygate dpool")   # 12 x 10 outputs, 240 px: tiles straddle images, 16 dead pixels
CASES["m7_tiny"] = _case(1, 5, 5, 7, 2, 3, 64, "notab")                     # map smaller than the kernel: every tap row clamps on both sides
CASES["m7_s1"] = _case(1, 8, 9, 7, 1, 3, 64)                                # stride 1
# 3. the direct kernels k_stem_fwd / k_stem_bwd<K,KR>
CASES["d3_c64"] = _case(2, 17, 19, 3, 2, 1, 64, "fin fold")                 # k_stem_bwd<3,3>
CASES["d3_c8"] = _case(2, 9, 9, 3, 2, 1, 8)                                 # one channel group (CG = 1; backward C4 = 2)
CASES["d3_c256"] = _case(1, 9, 9, 3, 2, 1, 256)                             # CG = 32, PL = 8; backward C4 = 64, PL = 4
CASES["d7_c32"] = _case(2, 13, 11, 7, 2, 3, 32, "ygate dpool")              # backward: seven launches of k_stem_bwd<7,1>
CASES["d1_c32"] = _case(2, 6, 10, 1, 1, 0, 32, "nocoef")                    # k_stem_bwd<1,1>
CASES["d5_c32"] = _case(2, 9, 9, 5, 2, 2, 32)                               # forward only; the backward refuses k = 5
BWD_CASES = [n for n, c in CASES.items() if c["k"] != 5]
NOSTATS_TWICE = ["m3_33x29", "m7_23x19", "d3_c64", "d5_c32"]

# large mean at the output (image 1000 + N(0,1), every feature's weights sum to 1): the MFMA forwards keep SHIFTED per-lane sums
OFFSET = {
    "off_m3": _case(2, 65, 65, 3, 2, 0, 32, "offset"),
    "off_m7": _case(2, 69, 69, 7, 2, 0, 64, "offset"),
}

# calls the library must refuse (non-zero status, the reason in lhn_last_error, nothing written); kind: the entry point
REFUSE = {
    "c24": _case(1, 9, 9, 3, 2, 1, 24, kind="fwd", refuse="Cout=24"),
    "k2": _case(1, 9, 9, 2, 1, 0, 32, kind="fwd", refuse="k=2"),
    "wrong_out": _case(1, 9, 9, 3, 2, 1, 32, "badout", kind="fwd", refuse="expected 5x5"),
    "lds_k7_c128": _case(1, 9, 9, 7, 2, 3, 128, kind="fwd", refuse="91648 B of LDS"),
    "lds_k7_c256": _case(1, 9, 9, 7, 2, 3, 256, kind="fwd", refuse="166912 B of LDS"),
    "lds_k5_c256": _case(1, 9, 9, 5, 2, 2, 256, kind="fwd", refuse="93184 B of LDS"),
    "bwd_k5": _case(2, 9, 9, 5, 2, 2, 32, kind="bwd", refuse="k=5"),
}
_ALL = dict(CASES, **OFFSET, **REFUSE)


def out_hw(c):
    f = lambda e: (e + 2 * c["p"] - c["k"]) // c["s"] + 1      # noqa: E731
    return f(c["hi"]), f(c["wi"])


def direct_lds(c):
    """Dynamic LDS of k_stem_fwd as lhn_conv_stem_fwd sizes it: the weights [3 k k][Cout] and 256 x 16 floats of reduction scratch."""
    return 3 * c["k"] * c["k"] * c["cout"] * 4 + 256 * 16 * 4


def kernel_of(name, gather=False, kind="fwd"):
    """The kernel lhn_conv_stem_fwd / lhn_conv_stem_bwd launch for a case (gather: under LHN_DW_GATHER=1)."""
    c = _ALL[name]
    k, co = c["k"], c["cout"]
    if k == 7 and co == 64 and not gather:
        return f"k_stem7_{kind}_mfma"
    if k == 3 and co == 32 and not gather:
        return f"k_stem3_{kind}_mfma"
    if kind == "fwd":
        return "k_stem_fwd"
    return {3: "k_stem_bwd<3,3>", 1: "k_stem_bwd<1,1>", 7: "k_stem_bwd<7,1> x 7"}[k]


def _gen(name, seed):
    c = _ALL[name]
    f, n, k, co, ycs = c["flags"], c["n"], c["k"], c["cout"], c["ycs"]
    ho, wo = out_hw(c)
    g = {"seed": seed}
    g["img"] = _rand((n, 3, c["hi"], c["wi"]), seed)
    g["w"] = _rand((co, 3, k, k), seed + 3, (3 * k * k) ** -0.5)
    if "offset" in f:
        g["img"] = g["img"] + 1000.0
        g["w"] = g["w"] - g["w"].mean(dim=(1, 2, 3), keepdim=True) + 1.0 / (3 * k * k)
        return g
    if "fin" in f:
        g["gamma"], g["beta"] = 1 + 0.2 * _rand((co,), seed + 60), 0.3 * _rand((co,), seed + 61)
        g["rmean"], g["rvar"] = 0.1 * _rand((co,), seed + 62), 1 + 0.2 * _rand((co,), seed + 63).abs()
        if "bias" in f:
            g["cbias"] = 0.5 * _rand((co,), seed + 64)
    # backward: y is an input (raw values under a table), whatever the forward of this image would have stored
    g["y"] = _rand((n, ho, wo, ycs), seed + 1)
    g["dz"] = _rand((n, ho, wo, ycs), seed + 2)
    if "notab" not in f:
        g["ytab"] = _tab(ycs, seed + 6)
    if "nocoef" not in f:
        g["coef"] = torch.stack([1 + 0.2 * _rand((ycs,), seed + 8), 0.1 * _rand((ycs,), seed + 9), 0.1 * _rand((ycs,), seed + 10)]).contiguous()
    if "ygate" in f:
        g["ygate"] = torch.sigmoid(_rand((n, ycs), seed + 12))
    if "dpool" in f:
        g["dpool"] = 0.3 * _rand((n, 25, ycs), seed + 13)
    g["prior"] = 0.5 * _rand((co * 3 * k * k,), seed + 14)      # what the gradient replicas hold before the call, summed
    return g


def inputs(name, seed=7):
    """Seeded inputs; a seed at which some activation input changes sign between float32 and float64 is passed over."""
    for s in range(seed, seed + 1000, 100):
        g = _gen(name, s)
        if "ytab" not in g or _kinks(g["y"], g["ytab"]) == 0:
            return g
    raise AssertionError(f"{name}: no seed without an activation kink")


# ---------------------------------------------------------------- kernels
def run_fwd(name, dev, g=None, stats=True, expect_fail=False, fin_separate=True):
    """Outputs of lhn_conv_stem_fwd as numpy arrays (the view's channels; the 32 statistics replicas folded on the host in float64),
    plus `*_ok` flags: every float outside the outputs still holds its prefill, bit for bit.  A `fin` case also runs lhn_bn_finalize as
    a launch of its own on the statistics the call left behind (`sep_*`, and `sep_bits_equal`: the two agree in every bit)."""
    c = _ALL[name]
    f, n, k, co, ycs, ycoff = c["flags"], c["n"], c["k"], c["cout"], c["ycs"], c["ycoff"]
    ho, wo = out_hw(c)
    if "badout" in f:
        ho += 1
    g = g or inputs(name)
    d = {kk: (v.to(dev) if torch.is_tensor(v) else v) for kk, v in g.items()}
    L, st = _lib.lib(), _lib.stream()
    y = torch.full((n, ho, wo, ycs), PREFILL, device=dev)
    vy = _view(y, ycoff, co)
    sbuf = torch.zeros(STAT_REPLICAS * 2 * co + STAT_PAD, dtype=torch.float64, device=dev) if stats else None
    fin, fb = None, {}
    if "fin" in f and stats:
        fb = {"counter": torch.zeros(TICKET_WORDS, dtype=torch.int32, device=dev), "table": torch.full((3, ycs), PREFILL, device=dev),
              "save": torch.full((2, co), PREFILL, device=dev), "rmean": d["rmean"].clone(), "rvar": d["rvar"].clone(),
              "nbt": torch.full((1,), 5, dtype=torch.int64, device=dev)}
        fin = BnFin()
        fin.counter, fin.gamma, fin.beta = fb["counter"].data_ptr(), d["gamma"].data_ptr(), d["beta"].data_ptr()
        fin.running_mean, fin.running_var, fin.num_batches_tracked = fb["rmean"].data_ptr(), fb["rvar"].data_ptr(), fb["nbt"].data_ptr()
        fin.table, fin.save_mean_invstd, fin.count = fb["table"].data_ptr(), fb["save"].data_ptr(), float(n * ho * wo)
        fin.cstride, fin.coff, fin.C, fin.eps, fin.momentum, fin.slope = ycs, ycoff, co, EPS, MOMENTUM, SLOPE
        fin.conv_bias = d["cbias"].data_ptr() if "cbias" in d else None
    rc = L.lhn_conv_stem_fwd(_lib.ptr(d["img"]), _lib.ptr(d["w"]), C.byref(vy), _lib.ptr(sbuf), c["hi"], c["wi"], k, c["s"], c["p"],
                             C.byref(fin) if fin is not None else None, st)
    torch.cuda.synchronize()
    if expect_fail:
        return rc, bool((y == PREFILL).all()) and bool((sbuf == 0).all())
    _lib.check(rc, f"stem fwd {name}")
    out = {"y": y[..., ycoff:ycoff + co].cpu().numpy(), "y_outside_ok": np.array(bool((_outside(y, ycoff, co) == PREFILL).all()))}
    if sbuf is not None:
        tot = sbuf[:STAT_REPLICAS * 2 * co].view(STAT_REPLICAS, 2, co).cpu().numpy().sum(0)
        out["stats_sum"], out["stats_sq"] = tot[0], tot[1]        # two outputs: each row against its own scale
        out["stats_pad_ok"] = np.array(bool((sbuf[STAT_REPLICAS * 2 * co:] == 0).all()))
    if fin is not None:
        tab = fb["table"][:, ycoff:ycoff + co].cpu().numpy()
        out["fin_scale"], out["fin_shift"], out["fin_slope"] = tab[0], tab[1], tab[2]
        out["fin_mean"], out["fin_invstd"] = fb["save"][0].cpu().numpy(), fb["save"][1].cpu().numpy()
        out["fin_rmean"], out["fin_rvar"] = fb["rmean"].cpu().numpy(), fb["rvar"].cpu().numpy()
        out["fin_nbt"] = fb["nbt"].cpu().numpy()
        out["table_outside_ok"] = np.array(bool((_outside(fb["table"], ycoff, co) == PREFILL).all()))
        if fin_separate:
            t2, s2 = torch.full((3, ycs), PREFILL, device=dev), torch.full((2, co), PREFILL, device=dev)
            rm2, rv2, nbt2 = d["rmean"].clone(), d["rvar"].clone(), torch.full((1,), 5, dtype=torch.int64, device=dev)
            _lib.check(L.lhn_bn_finalize(_lib.ptr(sbuf), _lib.ptr(d["gamma"]), _lib.ptr(d["beta"]), _lib.ptr(rm2), _lib.ptr(rv2), _lib.ptr(nbt2),
                                         _lib.ptr(t2), ycs, ycoff, co, _lib.ptr(s2), C.c_double(n * ho * wo), C.c_float(EPS),
                                         C.c_float(MOMENTUM), C.c_float(SLOPE), 1, _lib.ptr(d.get("cbias")), st), "bn finalize")
            torch.cuda.synchronize()
            same = all(torch.equal(a, b) for a, b in ((t2, fb["table"]), (s2, fb["save"]), (rm2, fb["rmean"]), (rv2, fb["rvar"]), (nbt2, fb["nbt"])))
            out["sep_bits_equal"] = np.array(same)
            out["sep_scale"], out["sep_shift"] = t2[0, ycoff:ycoff + co].cpu().numpy(), t2[1, ycoff:ycoff + co].cpu().numpy()
            out["sep_mean"], out["sep_invstd"] = s2[0].cpu().numpy(), s2[1].cpu().numpy()
            out["sep_rmean"], out["sep_rvar"] = rm2.cpu().numpy(), rv2.cpu().numpy()
    return out


def run_bwd(name, dev, g=None, expect_fail=False):
    """dW [Cout,3,k,k] of lhn_conv_stem_bwd: the _nrep(c) gradient replicas (each prefilled with its share of the prior) folded on
    the host in float64, or by lhn_reduce_replicas (`fold`); `*_ok` flags: the slack behind every replica, y and dz keep their bits."""
    c = _ALL[name]
    f, n, k, co, ycs, ycoff = c["flags"], c["n"], c["k"], c["cout"], c["ycs"], c["ycoff"]
    g = g or inputs(name)
    d = {kk: (v.to(dev) if torch.is_tensor(v) else v) for kk, v in g.items()}
    L, st = _lib.lib(), _lib.stream()
    y, dz = d["y"].clone(), d["dz"].clone()
    vy = _view(y, ycoff, co, d.get("ytab"), d.get("ygate"))
    gv = GradView()
    gv.dz, gv.dpool, gv.coef = dz.data_ptr(), (d["dpool"].data_ptr() if "dpool" in d else None), (d["coef"].data_ptr() if "coef" in d else None)
    nrep, tw = _nrep(c), co * 3 * k * k
    rs = tw + DW_SLACK
    gbuf = torch.full((nrep, rs), PREFILL, device=dev)
    gbuf[:, :tw] = d["prior"] / nrep                 # nrep is 4 or 16: the shares are exact and sum to the prior
    before = gbuf.clone()
    rc = L.lhn_conv_stem_bwd(_lib.ptr(d["img"]), C.byref(vy), C.byref(gv), _lib.ptr(gbuf), c["hi"], c["wi"], k, c["s"], c["p"], nrep,
                             C.c_int64(rs), st)
    torch.cuda.synchronize()
    if expect_fail:
        return rc, torch.equal(gbuf, before) and torch.equal(dz, d["dz"]) and torch.equal(y, d["y"])
    _lib.check(rc, f"stem bwd {name}")
    out = {"dw_pad_ok": np.array(bool((gbuf[:, tw:] == PREFILL).all())), "dz_ok": np.array(torch.equal(dz, d["dz"])),
           "y_ok": np.array(torch.equal(y, d["y"]))}
    if "fold" in f:
        dw = torch.full((tw + DW_SLACK,), PREFILL, device=dev)
        _lib.check(L.lhn_reduce_replicas(_lib.ptr(dw), _lib.ptr(gbuf), C.c_int64(tw), nrep, C.c_int64(rs), st), "reduce replicas")
        torch.cuda.synchronize()
        out["dw"] = dw[:tw].view(co, 3, k, k).cpu().numpy()
        out["fold_pad_ok"] = np.array(bool((dw[tw:] == PREFILL).all()))
    else:
        out["dw"] = gbuf[:, :tw].cpu().double().sum(0).view(co, 3, k, k).numpy()
    return out


def run(name, dev, g=None, kind="fwd", **kw):
    return run_fwd(name, dev, g, **kw) if kind == "fwd" else run_bwd(name, dev, g, **kw)


# ---------------------------------------------------------------- reference
def reference_fwd(name, g=None, dtype=torch.float64, stats=True):
    """conv2d of the image over zero padding; per-channel sum and sum of squares; the train-mode BatchNorm of y."""
    c = _ALL[name]
    f, co = c["flags"], c["cout"]
    g = g or inputs(name)
    y = F.conv2d(g["img"].to(dtype), g["w"].to(dtype), None, c["s"], c["p"]).permute(0, 2, 3, 1)
    out = {"y": y.double().numpy()}
    if stats:
        out["stats_sum"], out["stats_sq"] = y.sum((0, 1, 2)).double().numpy(), (y * y).sum((0, 1, 2)).double().numpy()
    if "fin" in f and stats:
        cnt = y.numel() // co
        mean, var = y.mean((0, 1, 2)), y.var((0, 1, 2), unbiased=False)
        invstd = 1.0 / torch.sqrt(var + EPS)
        scale = g["gamma"].to(dtype) * invstd
        cb = g["cbias"].to(dtype) if "cbias" in g else 0.0
        out["fin_scale"], out["fin_shift"] = scale.double().numpy(), (g["beta"].to(dtype) - mean * scale).double().numpy()
        out["fin_slope"] = np.full(co, np.float32(SLOPE), np.float64)
        out["fin_mean"], out["fin_invstd"] = mean.double().numpy(), invstd.double().numpy()
        out["fin_rmean"] = ((1 - MOMENTUM) * g["rmean"].to(dtype) + MOMENTUM * (mean + cb)).double().numpy()
        out["fin_rvar"] = ((1 - MOMENTUM) * g["rvar"].to(dtype) + MOMENTUM * var * cnt / (cnt - 1)).double().numpy()
    return out


def reference_bwd(name, g=None, dtype=torch.float64):
    """du = act'(u) * (gate * dz + pooled gradient of the pixel's segment), dy = A*du + B*y + C (include/lhn.h: lhn_gradview), then the
    plain weight gradient of the convolution, dW[co][c][kh][kw] = sum over pixels of dy[pixel][co] * padded image[c][tap], plus the prior."""
    c = _ALL[name]
    n, k, co = c["n"], c["k"], c["cout"]
    ho, wo = out_hw(c)
    g = g or inputs(name)
    ys = slice(c["ycoff"], c["ycoff"] + co)
    e = g["dz"][..., ys].to(dtype)
    if "ygate" in g:
        e = e * g["ygate"][:, ys].to(dtype)[:, None, None, :]
    if "dpool" in g:
        slot = torch.tensor([[_seg(i, ho) * 5 + _seg(j, wo) for j in range(wo)] for i in range(ho)])
        e = e + g["dpool"][:, :, ys].to(dtype)[:, slot.view(-1)].view(n, ho, wo, co)
    du = e * _dact(g["y"][..., ys], g["ytab"][:, ys], dtype) if "ytab" in g else e
    if "coef" in g:
        A, B, Cc = (g["coef"][i, ys].to(dtype) for i in range(3))
        dy = A * du + B * g["y"][..., ys].to(dtype) + Cc
    else:
        dy = du
    patch = F.unfold(g["img"].to(dtype), k, padding=c["p"], stride=c["s"])             # [n][3 k k][ho wo], rows in (c, kh, kw) order
    dw = torch.einsum("nlc,ntl->ct", dy.reshape(n, ho * wo, co), patch).reshape(co, 3, k, k)
    return {"dw": (dw + g["prior"].to(dtype).view(co, 3, k, k)).double().numpy()}


def reference(name, g=None, dtype=torch.float64, kind="fwd", **kw):
    return reference_fwd(name, g, dtype, **kw) if kind == "fwd" else reference_bwd(name, g, dtype)


def offset_premise(name, g=None):
    """(|mean| / sigma at the output, least over the channels; the float64 batch variance per channel) of a large-mean case."""
    y = torch.from_numpy(reference_fwd(name, g or inputs(name), stats=False)["y"])
    mean, var = y.mean((0, 1, 2)), y.var((0, 1, 2), unbiased=False)
    return float((mean.abs() / var.sqrt()).min()), var.numpy()


def _check_reference():
    import time
    t0, worst = time.time(), 0.0
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "litehandnet_amd", "csrc", "k_conv_stem.hip")).read()
    fwd_src = src[src.index('extern "C" int lhn_conv_stem_fwd'):src.index("stem backward (weight gradient")]
    bwd_src = src[src.index('extern "C" int lhn_conv_stem_bwd'):]
    for s, kind in ((fwd_src, "fwd"), (bwd_src, "bwd")):      # the two conditions kernel_of repeats, as the launchers spell them
        i7 = s.index("if (k == 7 && y->C == 64 && !lhn_dw_force_gather())")
        i3 = s.index("else if (k == 3 && y->C == 32 && !lhn_dw_force_gather())")
        assert i7 < s.index(f"k_stem7_{kind}_mfma,") < i3 < s.index(f"k_stem3_{kind}_mfma,"), kind
    for want in ("k_stem_bwd<3, 3>", "k_stem_bwd<1, 1>", "k_stem_bwd<7, 1>", "kh < 7"):
        assert want in bwd_src, want
    for nm, c in CASES.items():
        g = inputs(nm)
        assert g["seed"] == 7, f"{nm} needed seed {g['seed']}"
        assert "ytab" not in g or _kinks(g["y"], g["ytab"]) == 0
        for kind in ("fwd", "bwd") if nm in BWD_CASES else ("fwd",):
            r64, r32 = reference(nm, g, kind=kind), reference(nm, g, torch.float32, kind=kind)
            for k in r64:
                assert np.isfinite(r64[k]).all() and np.abs(r64[k]).max() > 0, f"{nm} {k}: reference not finite or all zeros"
                e = rel_err(r32[k], r64[k])
                assert np.isfinite(3 * e), f"{nm} {k}"
                worst = max(worst, e)
        mfma = (c["k"], c["cout"]) in ((3, 32), (7, 64))
        assert nm.startswith("m") == mfma and kernel_of(nm).endswith("_mfma") == mfma and not kernel_of(nm, True).endswith("_mfma"), nm
        assert mfma or direct_lds(c) <= DIRECT_LDS_LIMIT, nm
        print(f"{nm:10s} fwd {kernel_of(nm):18s} gather: {kernel_of(nm, True):12s}" +
              (f" bwd {kernel_of(nm, kind='bwd'):20s} gather: {kernel_of(nm, True, 'bwd')}" if nm in BWD_CASES else " bwd refused"))
    for nm, c in REFUSE.items():
        if nm.startswith("lds_"):
            assert direct_lds(c) > DIRECT_LDS_LIMIT and f"{direct_lds(c)} B" in c["refuse"], nm
    for nm in OFFSET:
        ratio, var = offset_premise(nm)
        assert ratio > 300 and np.isfinite(var).all(), (nm, ratio)
        print(f"{nm:10s} fwd {kernel_of(nm):18s} |mean| / sigma >= {ratio:.0f}")
    print(f"{len(CASES)} cases, no activation kinks at seed 7, worst float32 error {worst:.2e}, {time.time() - t0:.1f} s")


if __name__ == "__main__":
    if sys.argv[1] == "--check-reference":
        _check_reference()
        sys.exit(0)
    dst, reps, names = sys.argv[1], int(sys.argv[2]), sys.argv[3:]
    dev = torch.device("cuda:0")
    res = {}
    for full in names:
        kind, nm = full.split(":")
        g = inputs(nm)
        for r in range(reps):
            for k, v in run(nm, dev, g, kind=kind).items():
                res[f"{full}/{r}/{k}"] = v
    np.savez(dst, **res)
