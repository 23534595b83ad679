"""Cases of the 1x1 convolution (lhn_conv_pw_fwd2 / lhn_conv_pw_bwd3) run through the C ABI, with a plain torch reference on the
CPU (float64, or float32 to measure what the same operation loses in the kernels' own precision).  Imported by
tests/test_pw_gpu.py; run as a script (a child process with its own environment, e.g. LHN_PW_LDSW=1, LHN_PW_K256=0 or
LHN_DETERMINISTIC=1) it writes the kernel outputs of the named cases to an .npz file:
    python tests/pw_cases.py OUT.npz REPEATS fwd:NAME bwd:NAME ...
    python tests/pw_cases.py --check-reference        (CPU only: every case's inputs and both references)
    python tests/pw_cases.py --instances              (CPU only: prints profiles/pw_instances.md)
kernel_of(kind, name) asks the library which kernels a case launches (lhn_conv_pw_route: host only)."""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from litehandnet_amd import _lib  # noqa: E402
from litehandnet_amd._lib import GradView, View  # noqa: E402


class PwOpts(C.Structure):       # lhn_pw_opts (include/lhn.h)
    _fields_ = [("w_cols", C.c_int32), ("w_rows", C.c_int32), ("nchw_batch_stride", C.c_int64), ("n_extra", C.c_int32),
                ("extra", C.c_void_p), ("coef", C.c_float * 3), ("sum_out", C.c_void_p)]


class BnSum(C.Structure):        # lhn_bnsum (include/lhn.h)
    _fields_ = [("sums", C.c_void_p), ("save", C.c_void_p), ("C", C.c_int32), ("coff", C.c_int32)]


PREFILL = 7.0
COEF = (1.0, 0.5, -0.25)         # summed-on-load coefficients
HEAD_C, HEAD_ROWS, STACKS = 24, 21, 2      # the 21-joint head stored as 24 channels, stack 1 of 2


def _case(cin, cout, nhw, flags="", stride=1, **kw):
    return dict(cin=cin, cout=cout, nhw=nhw, flags=flags.split(), stride=stride, **kw)


# ---------------------------------------------------------------- forward table
# flags: xtab / xgate: pending transform / gate on x;  xview: x is channels [64, 64 + Cin) of a wider buffer;  yview: y is channels
# [32, 32 + Cout) of a wider buffer;  nostats;  bias;  nchw: NCHW store at the stacked batch stride;  extras1 / extras2: summed-on-load
# sources (each with its own table, the first one gated) with sum_out;  wmis: weight pointer 4 bytes off a 16-byte boundary
FWD = {}
for _ci, _co in ((32, 32), (32, 64), (32, 128), (64, 32), (64, 64), (64, 128), (128, 64), (128, 128)):
    FWD[f"wr_{_ci}_{_co}"] = _case(_ci, _co, (3, 9, 13), "xtab")                    # 351 px: no multiple of the 32/64/128-pixel tiles
FWD["wr_tiny_64_64"] = _case(64, 64, (1, 5, 7))                                     # 35 px: under one tile
FWD["wr_tiny_32_128"] = _case(32, 128, (1, 5, 7))
FWD["view_64_64"] = _case(64, 64, (2, 12, 20), "xtab xgate xview yview")
FWD["view_128_32"] = _case(128, 32, (2, 12, 20), "xtab xgate xview yview")
for _ci, _co in ((128, 64), (64, 64), (32, 32)):
    FWD[f"s2_{_ci}_{_co}_odd"] = _case(_ci, _co, (2, 11, 11), "xtab", stride=2)
    FWD[f"s2_{_ci}_{_co}_even"] = _case(_ci, _co, (1, 8, 10), "xtab", stride=2)
for _ci, _co in ((20, 20), (40, 80), (72, 72), (12, 24), (32, 40), (32, 96)):       # 72, 96: 3 of 4 feature tiles
    FWD[f"tail_{_ci}_{_co}"] = _case(_ci, _co, (2, 9, 11), "xtab")
for _ci, _co, _fl in ((160, 96, ""), (320, 40, "bias nostats"), (300, 60, ""), (256, 64, ""), (64, 256, "bias nostats"), (128, 256, ""),
                      (256, 32, "")):
    FWD[f"slice_{_ci}_{_co}"] = _case(_ci, _co, (2, 7, 9), "xtab " + _fl)
FWD["k256_256_256"] = _case(256, 256, (2, 10, 12), "xtab")
FWD["k256_256_128"] = _case(256, 128, (2, 10, 12), "xtab")
FWD["head_256_24"] = _case(256, HEAD_C, (3, 6, 6), "xtab nchw bias nostats", w_rows=HEAD_ROWS)   # HoWo = 36: 64-pixel tiles straddle images
FWD["head_64_24"] = _case(64, HEAD_C, (3, 6, 6), "xtab nchw bias nostats", w_rows=HEAD_ROWS)
FWD["head_24_256"] = _case(HEAD_C, 256, (3, 6, 6), "", w_cols=HEAD_ROWS)                         # pad channels of x hold NaN
FWD["ms_64_64_e1"] = _case(64, 64, (2, 9, 13), "xtab extras1")
FWD["ms_64_64_e2"] = _case(64, 64, (2, 9, 13), "xtab extras2")
FWD["ms_128_128_e2"] = _case(128, 128, (2, 9, 13), "xtab extras2")
FWD["ms_64_64_e2_wmis"] = _case(64, 64, (2, 9, 13), "xtab extras2 wmis")
FWD["big_32_32"] = _case(32, 32, (2, 257, 257), "nostats")                         # 132,098 px: more tiles than resident workgroups
FWD["big_64_64"] = _case(64, 64, (2, 257, 257))
FWD["big_128_128"] = _case(128, 128, (2, 257, 257), "nostats")

# ---------------------------------------------------------------- backward table
# always: x table, y table, coef, 4 weight-gradient replicas, dx prefilled 7.0.  flags: acc: dx holds a prior and is added to;
# dbias;  xgate / ygate / dpool;  views: x / dx are channels [64, 64 + Cin), y / dz channels [32, 32 + Cout) of wider buffers;
# nodx;  bns: reader-side BatchNorm sums (C = 128, coff = 64);  nchw: the head's NCHW gradient;  split: the host takes
# lhn_pw_bwd_split (dz is overwritten with dy);  stride 2 runs on a zeroed dx with accumulate
BWD = {}
for _i, (_ci, _co) in enumerate(((32, 32), (32, 64), (32, 128), (64, 32), (64, 64), (128, 32), (20, 20), (40, 80), (72, 72), (160, 40))):
    BWD[f"fused_{_ci}_{_co}"] = _case(_ci, _co, (3, 9, 13), ("acc " if _i % 2 else "") + ("dbias" if _i in (1, 9) else ""))
BWD["full_64_64"] = _case(64, 64, (2, 16, 19), "xgate ygate dpool acc views")
BWD["full_32_128"] = _case(32, 128, (2, 16, 19), "xgate ygate dpool acc views")
BWD["nodx_64_64"] = _case(64, 64, (2, 8, 8), "nodx")
BWD["nodx_128_128"] = _case(128, 128, (2, 8, 8), "nodx split")
BWD["s2_128_64"] = _case(128, 64, (2, 11, 11), "", stride=2)
BWD["s2_32_32"] = _case(32, 32, (2, 11, 11), "", stride=2)
for _ci, _co in ((64, 64), (32, 64), (64, 32)):
    BWD[f"bns_{_ci}_{_co}_16"] = _case(_ci, _co, (2, 16, 16), "bns")
    BWD[f"bns_{_ci}_{_co}_odd"] = _case(_ci, _co, (3, 9, 13), "bns")
BWD["head_256_24"] = _case(256, HEAD_C, (3, 6, 6), "nchw dbias", w_rows=HEAD_ROWS)
BWD["head_64_24"] = _case(64, HEAD_C, (3, 6, 6), "nchw dbias", w_rows=HEAD_ROWS)
# (dx is STORED into its prefill for one Cout = 256 and two Cin = 256 rows; three rows run on channel-slice views)
for _ci, _co, _nhw, _fl in ((64, 128, (2, 7, 9), "dbias"), (128, 64, (2, 24, 24), "acc"), (128, 128, (2, 7, 9), "acc"),
                            (256, 256, (2, 24, 24), "ygate dpool acc views"), (256, 128, (2, 7, 9), "ygate dpool dbias views"),
                            (128, 256, (2, 24, 24), "views"), (256, 64, (2, 7, 9), ""), (64, 256, (2, 24, 24), "acc"), (256, 32, (2, 7, 9), "")):
    BWD[f"split_{_ci}_{_co}"] = _case(_ci, _co, _nhw, "split " + _fl)
BWD["big_64_64"] = _case(64, 64, (2, 257, 257), "", nrep=16)
BWD["big_128_128"] = _case(128, 128, (2, 257, 257), "split", nrep=16)

# calls the library must refuse (non-zero status, an error text, nothing written)
FWD_REFUSE = {
    "extra_32_32": _case(32, 32, (2, 8, 8), "xtab extras1", refuse="unsupported channels"),               # no instantiation with summed-on-load sources
    "extras_stride2": _case(64, 64, (2, 8, 8), "xtab extras2", stride=2, refuse="extra sources need stride 1"),
    "sum_out_alone": _case(64, 64, (2, 8, 8), "xtab sumonly", refuse="sum_out without extra"),
}
BWD_REFUSE = {
    "s2_store": _case(32, 32, (2, 11, 11), "s2store", stride=2, refuse="only accumulates"),
    "bns_large": _case(64, 128, (2, 8, 8), "bns", refuse="BatchNorm sums ride"),                         # Cin * Cout = 8192
    "bns_xgate": _case(64, 64, (2, 8, 8), "bns xgate", refuse="BatchNorm sums ride"),
    "bns_stride2": _case(64, 64, (2, 8, 8), "bns", stride=2, refuse="BatchNorm sums ride"),
}
TABLES = {"fwd": FWD, "bwd": BWD}
_ALL = {"fwd": dict(FWD, **FWD_REFUSE), "bwd": dict(BWD, **BWD_REFUSE)}


# LHN_PW_F_* / LHN_PW_SW_* (include/lhn.h)
F_NCHW, F_STATS, F_EXTRA1, F_EXTRA2, F_SUM_OUT, F_BNSUM, F_FIN, F_GATESUM, F_NO_DX, F_DX_ACC, F_DZ_DEAD, F_UNALIGNED, F_DBIAS = \
    1, 2, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192
SW_LDSW, SW_K256, SW_BWD_NARROW, SW_BWD_SPLIT, SW_HEAD_STREAM, SW_DETERMINISTIC = 1, 2, 4, 8, 16, 32
# the settings a table of profiles/pw_instances.md is printed for: title, kernel_of keywords
SETTINGS = (("default dispatch", {}), ("`LHN_PW_LDSW=1`", {"ldsw": True}), ("`LHN_PW_K256=0`", {"k256": False}),
            ("`LHN_PW_BWD_NARROW=0`", {"narrow": False}), ("`LHN_PW_BWD_SPLIT=1`", {"split": True}),
            ("`LHN_HEAD_STREAM=0`", {"head_stream": False}), ("`LHN_DETERMINISTIC=1`", {"deterministic": True}))


def kernel_of(kind, name, extra=0, ldsw=False, k256=True, narrow=True, split=False, head_stream=True, deterministic=False):
    """The launches of lhn_conv_pw_fwd2 / lhn_conv_pw_bwd3 for a case, in order, asked of the library (lhn_conv_pw_route: host only).
    extra: further LHN_PW_F_* bits (F_FIN, F_DZ_DEAD).  The keywords are the switches: ldsw: LHN_PW_LDSW=1, k256=False: LHN_PW_K256=0,
    narrow=False: LHN_PW_BWD_NARROW=0, split: LHN_PW_BWD_SPLIT=1, head_stream=False: LHN_HEAD_STREAM=0, deterministic:
    LHN_DETERMINISTIC=1.  None: no kernel for the case."""
    c = _ALL[kind][name]
    f, (n, h, w) = c["flags"], c["nhw"]
    if kind == "fwd":       # the LHN_PW_F_* bits of the call run_fwd / run_bwd make
        feat = (F_NCHW * ("nchw" in f) | F_STATS * ("nostats" not in f) | F_EXTRA1 * ("extras1" in f) | F_EXTRA2 * ("extras2" in f) |
                F_SUM_OUT * ("extras1" in f or "extras2" in f or "sumonly" in f) | F_UNALIGNED * ("wmis" in f))
    else:
        acc = "nodx" not in f and ("acc" in f or (c["stride"] == 2 and "s2store" not in f))
        feat = (F_NCHW * ("nchw" in f) | F_BNSUM * ("bns" in f) | F_NO_DX * ("nodx" in f) | F_DX_ACC * acc | F_DBIAS * ("dbias" in f) |
                F_GATESUM * ("slices" in c))
    sw = (SW_LDSW * ldsw | SW_K256 * k256 | SW_BWD_NARROW * narrow | SW_BWD_SPLIT * split | SW_HEAD_STREAM * head_stream |
          SW_DETERMINISTIC * deterministic)
    r = _lib.lib().lhn_conv_pw_route(int(kind == "bwd"), n, h, w, c["cin"], c["cout"], c["stride"], c.get("w_rows", 0), c.get("w_cols", 0), feat | extra, sw)
    return r.decode() if r is not None else None


def _rand(shape, seed, scale=1.0):
    return torch.from_numpy((np.random.Generator(np.random.PCG64(seed)).standard_normal(shape) * scale).astype(np.float32))


def _tab(cs, seed):
    return torch.stack([1 + 0.3 * _rand((cs,), seed), 0.2 * _rand((cs,), seed + 1), torch.full((cs,), 0.1)]).contiguous()


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


def geometry(kind, name):
    """Buffer widths and channel offsets of a case: (xcs, xcoff, ycs, ycoff, Ho, Wo)."""
    c = _ALL[kind][name]
    f, (n, h, w) = c["flags"], c["nhw"]
    wide_x, wide_y = ("xview" in f or "views" in f), ("yview" in f or "views" in f)
    xcs, xcoff = (c["cin"] + 64, 64) if wide_x else (c["cin"], 0)
    ycs, ycoff = (c["cout"] + 32, 32) if wide_y else (c["cout"], 0)
    s = c["stride"]
    return xcs, xcoff, ycs, ycoff, (h + s - 1) // s, (w + s - 1) // s


def _kinks(raw, tab):
    """Elements whose activation branch differs between float32 and float64 arithmetic."""
    u32 = raw * tab[0] + tab[1]
    u64 = raw.double() * tab[0].double() + tab[1].double()
    return int(((u32 > 0) != (u64 > 0)).sum())


def _gen(kind, name, seed):
    c = _ALL[kind][name]
    f, (n, h, w), cin, cout = c["flags"], c["nhw"], c["cin"], c["cout"]
    xcs, xcoff, ycs, ycoff, ho, wo = geometry(kind, name)
    g = {"seed": seed}
    g["x"] = _rand((n, h, w, xcs), seed)
    wr, wc = c.get("w_rows", cout), c.get("w_cols", cin)
    g["w"] = _rand((wr, wc), seed + 3, cin ** -0.5)
    if kind == "bwd" or "xtab" in f:
        g["xtab"] = _tab(xcs, seed + 4)
    if "xgate" in f:
        g["xgate"] = torch.sigmoid(_rand((n, xcs), seed + 11))
    if "bias" in f:
        g["bias"] = _rand((wr,), seed + 16)
    if kind == "fwd":
        if wc < cin:
            g["x"][..., xcoff + wc:xcoff + cin] = float("nan")
        ne = 1 if "extras1" in f else 2 if "extras2" in f else 0
        for e in range(ne):
            g[f"e{e}"] = _rand((n, h, w, cin), seed + 30 + e)
            g[f"e{e}tab"] = _tab(cin, seed + 40 + 2 * e)
        if ne:
            g["e0gate"] = torch.sigmoid(_rand((n, cin), seed + 50))
        return g
    g["y"] = _rand((n, ho, wo, ycs), seed + 1)
    g["ytab"] = _tab(ycs, seed + 6)
    if "nchw" in f:
        g["dy_nchw"] = _rand((n, STACKS, cout, ho * wo), seed + 2)        # both stacks and the three pad channels hold values
    else:
        g["dz"] = _rand((n, ho, wo, ycs), seed + 2)
        g["coef"] = torch.stack([1 + 0.2 * _rand((ycs,), seed + 8), 0.1 * _rand((ycs,), seed + 9), 0.1 * _rand((ycs,), seed + 10)]).contiguous()
    if "ygate" in f:
        g["ygate"] = torch.sigmoid(_rand((n, ycs), seed + 12))
    if "dpool" in f:
        g["dpool"] = 0.3 * _rand((n, 25, ycs), seed + 13)
    if "acc" in f:
        g["prior"] = _rand((n, h, w, xcs), seed + 14)
    if "bns" in f:
        g["save"] = torch.stack([0.1 * _rand((128,), seed + 20), 1 + 0.2 * _rand((128,), seed + 21).abs()]).contiguous()
    return g


def inputs(kind, name, seed=7):
    """Seeded inputs; a seed at which some activation input changes sign between float32 and float64 is passed over."""
    for s in range(seed, seed + 1000, 100):
        g = _gen(kind, name, s)
        bad = sum(_kinks(torch.nan_to_num(g[k]), g[k + "tab"]) for k in ("x", "y", "e0", "e1") if k in g and k + "tab" in g)
        if bad == 0:
            return g
    raise AssertionError(f"{kind}:{name}: no seed without an activation kink")


def _nrep(c):
    if os.environ.get("LHN_DETERMINISTIC") == "1":
        return 16        # deterministic mode: one gradient replica per workgroup, as the plan runs it
    return c.get("nrep", 4)


def _outside(t, coff, c):
    return torch.cat([t[..., :coff], t[..., coff + c:]], -1)


# ---------------------------------------------------------------- kernels
def run_fwd(name, dev, g=None, stats=None, expect_fail=False):
    """Outputs of lhn_conv_pw_fwd2 as numpy arrays (the view's channels), plus `*_ok` flags: every float outside the views
    still holds its prefill, bit for bit.  stats=False switches the statistics off for a case that has them."""
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
    wflat = torch.zeros(d["w"].numel() + 4, device=dev)
    woff = 1 if "wmis" in f else 0
    wflat[woff:woff + d["w"].numel()] = d["w"].reshape(-1)
    wptr = C.c_void_p(wflat.data_ptr() + 4 * woff)
    sbuf = torch.zeros(32, 2, cout, dtype=torch.float64, device=dev) if with_stats else None
    ynchw = torch.full((n, STACKS, cout, ho * wo), PREFILL, device=dev) if "nchw" in f else None
    o = PwOpts()
    o.w_cols, o.w_rows = c.get("w_cols", 0), c.get("w_rows", 0)
    o.nchw_batch_stride = STACKS * cout * ho * wo if ynchw is not None else 0
    ne = 1 if "extras1" in f else 2 if "extras2" in f else 0
    keep = []
    if ne:
        ev = (View * ne)(*[_view(d[f"e{e}"], 0, cin, d[f"e{e}tab"], d.get(f"e{e}gate")) for e in range(ne)])
        so = torch.full((n, h, w, cin + 64), PREFILL, device=dev)
        sv = _view(so, 64, cin)
        o.n_extra, o.extra, o.sum_out = ne, C.addressof(ev), C.addressof(sv)
        for i in range(3):
            o.coef[i] = COEF[i]
        keep += [ev, sv]
    if "sumonly" in f:
        so = torch.full((n, h, w, cin + 64), PREFILL, device=dev)
        sv = _view(so, 64, cin)
        o.sum_out = C.addressof(sv)
        keep += [sv]
    rc = L.lhn_conv_pw_fwd2(C.byref(vx), wptr, _lib.ptr(d.get("bias")), C.byref(vy), _lib.ptr(sbuf), stride,
                            C.c_void_p(ynchw[:, 1].data_ptr()) if ynchw is not None else None, None, C.byref(o), st)
    torch.cuda.synchronize()
    if expect_fail:
        return rc, bool((y == PREFILL).all()) and (not (ne or "sumonly" in f) or bool((so == PREFILL).all()))
    _lib.check(rc, f"pw fwd {name}")
    out = {}
    if ynchw is not None:
        out["y_nchw"] = ynchw[:, 1].cpu().numpy()
        out["nchw_other_ok"] = np.array(bool((ynchw[:, 0] == PREFILL).all()) and bool((y == PREFILL).all()))
    else:
        out["y"] = y[..., ycoff:ycoff + cout].cpu().numpy()
        out["y_outside_ok"] = np.array(bool((_outside(y, ycoff, cout) == PREFILL).all()))
    if sbuf is not None:
        tot = sbuf.sum(0).cpu().numpy()
        out["stats_sum"], out["stats_sq"] = tot[0], tot[1]        # two outputs: each row against its own scale
    if ne:
        out["sum_out"] = so[..., 64:64 + cin].cpu().numpy()
        out["sum_outside_ok"] = np.array(bool((_outside(so, 64, cin) == PREFILL).all()))
    return out


def run_bwd(name, dev, g=None, expect_fail=False):
    """Outputs of lhn_conv_pw_bwd3: dx (the view's channels), dW (replicas summed, [w_rows][w_cols]), dbias, BatchNorm sums, dz of
    the view after the call for the split path; `*_ok` flags: floats that must keep their bits did."""
    c = _ALL["bwd"][name]
    f, (n, h, w), cin, cout, stride = c["flags"], c["nhw"], c["cin"], c["cout"], c["stride"]
    xcs, xcoff, ycs, ycoff, ho, wo = geometry("bwd", name)
    g = g or inputs("bwd", name)
    d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in g.items()}
    L, st = _lib.lib(), _lib.stream()
    vx = _view(d["x"], xcoff, cin, d["xtab"], d.get("xgate"))
    vy = _view(d["y"], ycoff, cout, d["ytab"], d.get("ygate"))
    nchw = "nchw" in f
    dz = d["dz"].clone() if not nchw else None      # a fresh clone per call: the split path consumes it
    gv = GradView()
    gv.dz, gv.dpool = (dz.data_ptr() if dz is not None else None), (d["dpool"].data_ptr() if "dpool" in d else None)
    gv.coef = d["coef"].data_ptr() if "coef" in d else None
    wr, wc = c.get("w_rows", cout), c.get("w_cols", cin)
    nrep = _nrep(c)
    rs = cout * wc + cout + 16                       # one replica: dW laid out for all `cout` rows | dbias | slack
    gbuf = torch.zeros(nrep, rs, device=dev)
    dbp = C.c_void_p(gbuf.data_ptr() + 4 * cout * wc) if "dbias" in f else None
    if "nodx" in f:
        dx, acc = None, 0
    elif stride == 2:
        dx, acc = torch.zeros((n, h, w, xcs), device=dev), int("s2store" not in f)
    elif "prior" in d:
        dx, acc = d["prior"].clone(), 1
    else:
        dx, acc = torch.full((n, h, w, xcs), PREFILL, device=dev), 0
    o = PwOpts()
    o.w_cols, o.w_rows = c.get("w_cols", 0), c.get("w_rows", 0)
    o.nchw_batch_stride = STACKS * cout * ho * wo if nchw else 0
    bs, sums = None, None
    if "bns" in f:
        sums = torch.zeros(32, 2, 128, dtype=torch.float64, device=dev)
        bs = BnSum()
        bs.sums, bs.save, bs.C, bs.coff = sums.data_ptr(), d["save"].data_ptr(), 128, 64
    wdev = d["w"].contiguous()
    rc = L.lhn_conv_pw_bwd3(C.byref(vx), _lib.ptr(wdev), C.byref(vy), C.byref(gv), _lib.ptr(dx), acc, _lib.ptr(gbuf), dbp, stride,
                            C.c_void_p(d["dy_nchw"][:, 1].data_ptr()) if nchw else None, nrep, C.c_int64(rs), C.byref(o),
                            C.byref(bs) if bs is not None else None, st)
    torch.cuda.synchronize()
    if expect_fail:
        return rc, bool((gbuf == 0).all()) and torch.equal(dz, d["dz"]) and bool((dx == (0.0 if stride == 2 else PREFILL)).all()) and \
            (sums is None or bool((sums == 0).all()))
    _lib.check(rc, f"pw bwd {name}")
    out = {}
    tot = gbuf.sum(0)
    out["dw"] = tot[:wr * wc].view(wr, wc).cpu().numpy()
    out["dw_pad_ok"] = np.array(bool((gbuf[:, wr * wc:cout * wc] == 0).all()) and bool((gbuf[:, cout * wc + (cout if dbp else 0):] == 0).all()))
    if dbp:
        out["dbias"] = tot[cout * wc:cout * wc + wr].cpu().numpy()
        out["dw_pad_ok"] = np.array(bool(out["dw_pad_ok"]) and bool((gbuf[:, cout * wc + wr:] == 0).all()))
    if dx is not None:
        out["dx"] = dx[..., xcoff:xcoff + cin].cpu().numpy()
        before = d["prior"] if "prior" in d else torch.full_like(dx, 0.0 if stride == 2 else PREFILL)
        out["dx_outside_ok"] = np.array(torch.equal(_outside(dx, xcoff, cin), _outside(before, xcoff, cin)))
    if dz is not None:
        if "split" in f:
            out["dz"] = dz[..., ycoff:ycoff + cout].cpu().numpy()
            out["dz_outside_ok"] = np.array(torch.equal(_outside(dz, ycoff, cout), _outside(d["dz"], ycoff, cout)))
        else:
            out["dz_outside_ok"] = np.array(torch.equal(dz, d["dz"]))        # the fused kernel only reads dz
    if sums is not None:
        tot = sums.sum(0)[:, 64:64 + cin].cpu().numpy()
        out["sums_du"], out["sums_duxhat"] = tot[0], tot[1]
        out["sums_outside_ok"] = np.array(bool((_outside(sums, 64, cin) == 0).all()))
    return out


# ---------------------------------------------------------------- references
def _value(raw, tab, gate, dt):
    v = raw.to(dt)
    if tab is not None:
        u = v * tab[0].to(dt) + tab[1].to(dt)
        v = torch.where(u > 0, u, u * tab[2].to(dt))
    if gate is not None:
        v = v * gate.to(dt)[:, None, None, :]
    return v


def _dact(raw, tab, dt):
    u = raw.to(dt) * tab[0].to(dt) + tab[1].to(dt)
    return torch.where(u > 0, torch.ones_like(u), tab[2].to(dt).expand_as(u))


def reference_fwd(name, g=None, dtype=torch.float64, stats=None):
    c = _ALL["fwd"][name]
    f, (n, h, w), cin, cout, s = c["flags"], c["nhw"], c["cin"], c["cout"], c["stride"]
    xcs, xcoff, ycs, ycoff, ho, wo = geometry("fwd", name)
    g = g or inputs("fwd", name)
    sl = slice(xcoff, xcoff + cin)
    cut = lambda t: (t[..., sl] if t is not None else None)  # noqa: E731
    X = _value(g["x"][..., sl], cut(g.get("xtab")), cut(g.get("xgate")), dtype)
    ne = 1 if "extras1" in f else 2 if "extras2" in f else 0
    out = {}
    if ne:
        X = COEF[0] * X
        for e in range(ne):
            X = X + COEF[e + 1] * _value(g[f"e{e}"], g[f"e{e}tab"], g.get(f"e{e}gate"), dtype)
        out["sum_out"] = X.double().numpy()
    wt = g["w"].to(dtype)
    wr, wc = wt.shape
    y = X[:, ::s, ::s, :wc].reshape(-1, wc) @ wt.t()
    if "bias" in g:
        y = y + g["bias"].to(dtype)
    if wr < cout:                   # rows beyond the weight tensor: the kernel stores zeros (zero weights, zero bias)
        y = torch.cat([y, torch.zeros(y.shape[0], cout - wr, dtype=dtype)], 1)
    if "nchw" in f:
        out["y_nchw"] = y.view(n, ho * wo, cout).permute(0, 2, 1).double().numpy()
    else:
        out["y"] = y.view(n, ho, wo, cout).double().numpy()
    if ("nostats" not in f) if stats is None else stats:
        out["stats_sum"], out["stats_sq"] = y.sum(0).double().numpy(), (y * y).sum(0).double().numpy()
    return out


def reference_bwd(name, g=None, dtype=torch.float64):
    c = _ALL["bwd"][name]
    f, (n, h, w), cin, cout, s = c["flags"], c["nhw"], c["cin"], c["cout"], c["stride"]
    xcs, xcoff, ycs, ycoff, ho, wo = geometry("bwd", name)
    g = g or inputs("bwd", name)
    xs, ys = slice(xcoff, xcoff + cin), slice(ycoff, ycoff + cout)
    X = _value(g["x"][..., xs], g["xtab"][:, xs], g["xgate"][:, xs] if "xgate" in g else None, dtype)[:, ::s, ::s]
    wt = g["w"].to(dtype)
    wr, wc = wt.shape
    out = {}
    if "nchw" in f:
        dy = g["dy_nchw"][:, 1, :wr].to(dtype).permute(0, 2, 1).reshape(n, ho, wo, wr)
    else:
        e = g["dz"][..., ys].to(dtype)
        if "ygate" in g:
            e = e * g["ygate"][:, ys].to(dtype)[:, None, None, :]
        if "dpool" in g:
            slot = torch.tensor([[_seg(i, ho) * 5 + _seg(j, wo) for j in range(wo)] for i in range(ho)])
            e = e + g["dpool"][:, :, ys].to(dtype)[:, slot.view(-1)].view(n, ho, wo, cout)
        du = e * _dact(g["y"][..., ys], g["ytab"][:, ys], dtype)
        A, B, Cc = (g["coef"][i, ys].to(dtype) for i in range(3))
        dy = A * du + B * g["y"][..., ys].to(dtype) + Cc
        if "split" in f:
            out["dz"] = dy.double().numpy()
    dy2 = dy.reshape(-1, wr)
    out["dw"] = (dy2.t() @ X.reshape(-1, cin)[:, :wc]).double().numpy()
    if "dbias" in f:
        out["dbias"] = dy2.sum(0).double().numpy()
    if "nodx" not in f:
        dxs = (dy2 @ wt).view(n, ho, wo, wc)
        dxv = torch.zeros(n, h, w, cin, dtype=dtype)
        dxv[:, ::s, ::s, :wc] = dxs
        out["dx"] = (dxv + g["prior"][..., xs].to(dtype) if "prior" in g else dxv).double().numpy()
        if "bns" in f:
            mean, inv = g["save"][0, 64:64 + cin].to(dtype), g["save"][1, 64:64 + cin].to(dtype)
            du_x = dxv * _dact(g["x"][..., xs], g["xtab"][:, xs], dtype)
            out["sums_du"] = du_x.sum((0, 1, 2)).double().numpy()
            out["sums_duxhat"] = (du_x * (g["x"][..., xs].to(dtype) - mean) * inv).sum((0, 1, 2)).double().numpy()
    return out


def run(kind, name, dev, g=None):
    return run_fwd(name, dev, g) if kind == "fwd" else run_bwd(name, dev, g)


def reference(kind, name, g=None, dtype=torch.float64):
    return reference_fwd(name, g, dtype) if kind == "fwd" else reference_bwd(name, g, dtype)


def rel_err(a, b):
    """Max absolute difference over every element, relative to the reference's largest magnitude."""
    return float(np.abs(np.asarray(a, np.float64) - b).max()) / max(float(np.abs(b).max()), 1e-30)


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
    """profiles/pw_instances.md: one table per direction and switch setting; under a switch only the cases that change their launches."""
    print("# 1x1 convolution kernels: which test case launches what\n")
    print("The answers of `lhn_conv_pw_route` (`include/lhn.h`: host only, the route functions every `lhn_conv_pw_*` entry asks) for `FWD` / `BWD` of\n"
          "`tests/pw_cases.py`, printed by `python tests/pw_cases.py --instances`; `tests/test_pw_route_cpu.py` holds them as a literal table.\n"
          "Names as a kernel trace prints the template instances, launches in order; ` x n`: a launch that repeats (channel slices).")
    for kind, title in (("fwd", "Forward"), ("bwd", "Backward")):
        base = {nm: kernel_of(kind, nm) for nm in TABLES[kind]}
        for setting, kw in SETTINGS:
            got = {nm: kernel_of(kind, nm, **kw) for nm in TABLES[kind]}
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
    none = [f"{kind}:{nm}" for kind, tab in (("fwd", FWD_REFUSE), ("bwd", BWD_REFUSE)) for nm in tab if kernel_of(kind, nm) is None]
    print(", ".join(none))


if __name__ == "__main__":
    if sys.argv[1] == "--check-reference":
        _check_reference()
        sys.exit(0)
    if sys.argv[1] == "--instances":
        _instances()
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
