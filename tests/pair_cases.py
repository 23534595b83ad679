"""Cases of tests/test_pair_kernels_gpu.py: every two-job entry point (lhn_*_pair, lhn_bn_finalize_pair; include/lhn.h) against the two
single calls it stands for, on fresh copies of the same seeded inputs.  run(case, dev, pair) returns EVERY buffer either form may
write, whole (the prefilled floats around the views included), as numpy arrays; the test compares the two dictionaries bit for bit.
The single entries are the reference: tests/test_ew_pool_gpu.py and tests/test_bn_gpu.py hold them to float64.

    python tests/pair_cases.py OUT.npz [CASE ...]      child of the deterministic test: both forms of every case into one .npz

All at N = 2, the smallest shapes that reach every path: ceil-mode odd edges, views at channel offsets of shared and of separate
buffers, gates and tables on one job only, store and accumulate, both flush paths of the BatchNorm sums (8 channels: shuffles and
atomics; 20: LDS), a 64-pixel bin (the workgroup average-pool kernel)."""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ew_pool_cases import GradAdds  # noqa: E402
from pw_cases import PREFILL, BnSum, _lib, _rand, _view, rel_err  # noqa: E402,F401

REPLICAS = 32                    # LHN_STAT_REPLICAS
N = 2


class MaxpoolJob(C.Structure):   # lhn_maxpool_job
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("dy", C.c_void_p), ("dx", C.c_void_p), ("dx_accumulate", C.c_int32),
                ("bns", C.c_void_p), ("adds", C.c_void_p)]


class EwJob(C.Structure):        # lhn_ew_job
    _fields_ = [("srcs", C.c_void_p), ("nsrc", C.c_int32), ("coef", C.c_void_p), ("dst", C.c_void_p), ("out_slope", C.c_float),
                ("mode", C.c_int32), ("ddst", C.c_void_p), ("dst_dpool", C.c_void_p), ("dsrcs", C.c_void_p), ("accumulate", C.c_void_p),
                ("bns", C.c_void_p)]


class AvgpoolJob(C.Structure):   # lhn_avgpool_job
    _fields_ = [("x", C.c_void_p), ("out", C.c_void_p), ("OH", C.c_int32), ("OW", C.c_int32), ("out_cstride", C.c_int32),
                ("out_coff", C.c_int32), ("pstat", C.c_void_p), ("slices", C.c_void_p), ("copy_src", C.c_void_p)]


class BnFin(C.Structure):        # lhn_bnfin
    _fields_ = [("counter", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("running_mean", C.c_void_p),
                ("running_var", C.c_void_p), ("num_batches_tracked", C.c_void_p), ("table", C.c_void_p), ("save_mean_invstd", C.c_void_p),
                ("count", C.c_double), ("cstride", C.c_int32), ("coff", C.c_int32), ("C", C.c_int32),
                ("eps", C.c_float), ("momentum", C.c_float), ("slope", C.c_float), ("conv_bias", C.c_void_p)]


CASES = ["maxpool_fwd", "maxpool_bwd_c8", "maxpool_bwd_c20", "ew_fwd", "ew_bwd", "ew_bwd_dpool", "ew_bwd_multi", "avgpool_c8", "avgpool_c20",
         "finalize_train", "finalize_eval"]
# case -> {name of a sums output: (name of the stored gradient it was formed from, ...)}: see sums_reference
SUMS = {"maxpool_bwd_c8": "sums1", "maxpool_bwd_c20": "sums1", "ew_bwd": "sums0", "ew_bwd_dpool": "sums0", "ew_bwd_multi": "sums1"}


def _t(dev, shape, seed, scale=1.0):
    return _rand(shape, seed, scale).to(dev)


def _tab(dev, cs, seed, slope=0.1):
    return torch.stack([1 + 0.3 * _rand((cs,), seed), 0.2 * _rand((cs,), seed + 1), torch.full((cs,), slope)]).contiguous().to(dev)


def _gate(dev, cs, seed):
    return (0.25 + _rand((N, cs), seed).abs()).contiguous().to(dev)


def _full(dev, shape, dtype=torch.float32):
    return torch.full(shape, PREFILL, device=dev, dtype=dtype)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _np(t):
    return t.detach().cpu().numpy().copy()


def _bns(dev, cp, coff, seed):
    """Zeroed replicated sums and a saved mean | invstd of a producer with cp channels; the view starts at its channel coff."""
    sums = torch.zeros(REPLICAS, 2, cp, device=dev, dtype=torch.float64)
    save = torch.cat([0.1 * _rand((cp,), seed), 0.5 + _rand((cp,), seed + 1).abs()]).contiguous().to(dev)
    b = BnSum()
    b.sums, b.save, b.C, b.coff = sums.data_ptr(), save.data_ptr(), cp, coff
    return sums, save, b


def _call(L, pair, pair_fn, a, b, single):
    s = _lib.stream()
    if pair:
        return pair_fn(C.byref(a), C.byref(b), s)
    rc = single(a, s)
    return rc if rc else single(b, s)


def _maxpool_fwd(dev, pair, h=7, w=9, hb=None, overlap=False):
    L, c = _lib.lib(), 8
    xa, xb = _t(dev, (N, h, w, 8), 11), _t(dev, (N, hb or h, w, 24), 12)
    ta, ga = _tab(dev, 8, 13), _gate(dev, 8, 14)
    y = _full(dev, (N, (h + 1) // 2, (w + 1) // 2, 16))
    yb = y if hb is None else _full(dev, (N, (hb + 1) // 2, (w + 1) // 2, 16))
    va, vb = _view(xa, 0, c, ta, ga), _view(xb, 8, c)
    wa, wb = _view(y, 0, c), _view(yb, 4 if overlap else 8, c)
    ja, jb = MaxpoolJob(), MaxpoolJob()
    ja.x, ja.y, jb.x, jb.y = C.addressof(va), C.addressof(wa), C.addressof(vb), C.addressof(wb)
    rc = _call(L, pair, L.lhn_maxpool2_fwd_pair, ja, jb, lambda j, s: L.lhn_maxpool2_fwd(C.c_void_p(j.x), C.c_void_p(j.y), s))
    return rc, {"y": _np(y), "yb": _np(yb)}


def _maxpool_bwd(dev, pair, c):
    L, h, w = _lib.lib(), 8, 12
    # job 0: gated and tabled x at channel offset c of a 2c buffer, both addends (3 x 3 bins of an 8 x 12 map overlap), store
    x0, t0, g0 = _t(dev, (N, h, w, 2 * c), 21), _tab(dev, 2 * c, 22), _gate(dev, 2 * c, 23)
    y0, dy0, dx0 = _full(dev, (N, h // 2, w // 2, c)), _t(dev, (N, h // 2, w // 2, c), 24), _full(dev, (N, h, w, 2 * c))
    same, pooled = _t(dev, (N, h, w, c + 4), 25), _t(dev, (N, 3, 3, c + 8), 26)
    ad = GradAdds()
    ad.same, ad.same_cstride, ad.same_coff = same.data_ptr(), c + 4, 4
    ad.pooled, ad.OH, ad.OW, ad.pooled_cstride, ad.pooled_coff = pooled.data_ptr(), 3, 3, c + 8, 4
    # job 1: ungated x with a table, the producer's BatchNorm sums (its channels [4, 4 + c) of c + 4), accumulate
    x1, t1 = _t(dev, (N, h, w, c), 31), _tab(dev, c, 32)
    y1, dy1, dx1 = _full(dev, (N, h // 2, w // 2, c)), _t(dev, (N, h // 2, w // 2, c), 33), _t(dev, (N, h, w, c), 34)
    sums1, save1, b1 = _bns(dev, c + 4, 4, 35)
    v0, w0, v1, w1 = _view(x0, c, c, t0, g0), _view(y0, 0, c), _view(x1, 0, c, t1), _view(y1, 0, c)
    ja, jb = MaxpoolJob(), MaxpoolJob()
    ja.x, ja.y, ja.dy, ja.dx, ja.dx_accumulate, ja.adds = C.addressof(v0), C.addressof(w0), dy0.data_ptr(), dx0.data_ptr(), 0, C.addressof(ad)
    jb.x, jb.y, jb.dy, jb.dx, jb.dx_accumulate, jb.bns = C.addressof(v1), C.addressof(w1), dy1.data_ptr(), dx1.data_ptr(), 1, C.addressof(b1)
    single = lambda j, s: L.lhn_maxpool2_bwd3(C.c_void_p(j.x), C.c_void_p(j.y), C.c_void_p(j.dy), C.c_void_p(j.dx), j.dx_accumulate,      # noqa: E731
                                              C.c_void_p(j.bns), C.c_void_p(j.adds), s)
    rc = _call(L, pair, L.lhn_maxpool2_bwd_pair, ja, jb, single)
    out = {"dx0": _np(dx0), "dx1": _np(dx1), "sums1": _np(sums1), "y0": _np(y0), "y1": _np(y1)}
    # for sums_reference: the routed gradient of job 1 alone (a store into a scratch buffer by the single entry), x1, its table, save
    r1 = _full(dev, (N, h, w, c))
    _lib.check(L.lhn_maxpool2_bwd3(C.byref(v1), C.byref(w1), _p(dy1), _p(r1), 0, None, None, _lib.stream()), "maxpool routed gradient")
    out.update({"ref.g": _np(r1), "ref.raw": _np(x1), "ref.table": _np(t1), "ref.save": _np(save1), "ref.coff": np.int64(4)})
    return rc, out


def _ew_fwd(dev, pair, mode=0):
    L, c, h, w = _lib.lib(), 8, 8, 12
    dst = _full(dev, (N, h, w, 16))
    # job 0: same-resolution source gated, upsampled source plain, no coefficients, slope 1; job 1: the upsampled source gated and
    # tabled, coefficients, slope 0
    a0, a1, g0 = _t(dev, (N, h, w, 8), 41), _t(dev, (N, h // 2, w // 2, 16), 42), _gate(dev, 8, 43)
    b0, b1, g1, t1 = _t(dev, (N, h, w, 24), 44), _t(dev, (N, h // 2, w // 2, 8), 45), _gate(dev, 8, 46), _tab(dev, 8, 47)
    sa = (_lib.View * 2)(_view(a0, 0, c, None, g0), _view(a1, 8, c))
    sb = (_lib.View * 2)(_view(b0, 16, c), _view(b1, 0, c, t1, g1))
    da, db = _view(dst, 0, c), _view(dst, 8, c)
    coef = (C.c_float * 3)(1.0, 0.5, 0.0)
    ja, jb = EwJob(), EwJob()
    ja.srcs, ja.nsrc, ja.dst, ja.out_slope, ja.mode = C.addressof(sa), 2, C.addressof(da), 1.0, 0
    jb.srcs, jb.nsrc, jb.coef, jb.dst, jb.out_slope, jb.mode = C.addressof(sb), 2, C.addressof(coef), C.addressof(db), 0.0, mode
    single = lambda j, s: L.lhn_ew_fwd3(C.c_void_p(j.srcs), j.nsrc, C.c_void_p(j.coef), C.c_void_p(j.dst), C.c_float(j.out_slope), j.mode, s)      # noqa: E731
    rc = _call(L, pair, L.lhn_ew_fwd_pair, ja, jb, single)
    return rc, {"dst": _np(dst)}


def _ew_bwd(dev, pair, dpool):
    L, c, h, w = _lib.lib(), 8, 4, 6            # sources 4 x 6, destinations 8 x 12: fan-out 2 x 2
    # job 0: sums, store, leaky destination (reads its stored sign); job 1: no sums, accumulate, slope 1, a gated destination (with its
    # pooled gradient in the dpool case)
    s0, t0, d0, dd0 = _t(dev, (N, h, w, 16), 51), _tab(dev, 16, 52), _t(dev, (N, 2 * h, 2 * w, 8), 53), _t(dev, (N, 2 * h, 2 * w, 8), 54)
    ds0 = _full(dev, (N, h, w, 16))
    sums0, save0, bs0 = _bns(dev, 12, 4, 55)
    s1, d1, dd1, g1 = _t(dev, (N, h, w, 8), 56), _t(dev, (N, 2 * h, 2 * w, 24), 57), _t(dev, (N, 2 * h, 2 * w, 24), 58), _gate(dev, 24, 59)
    ds1 = _t(dev, (N, h, w, 8), 60)
    dp1 = _t(dev, (N, 25, 24), 61) if dpool else None
    vs0, vd0, vs1, vd1 = _view(s0, 8, c, t0), _view(d0, 0, c), _view(s1, 0, c), _view(d1, 16, c, None, g1)
    ja, jb = EwJob(), EwJob()
    dsa, dsb, aa, ab = (C.c_void_p * 1)(ds0.data_ptr()), (C.c_void_p * 1)(ds1.data_ptr()), (C.c_int * 1)(0), (C.c_int * 1)(1)
    bpa = (C.c_void_p * 1)(C.addressof(bs0))
    ja.srcs, ja.nsrc, ja.dst, ja.out_slope, ja.ddst, ja.dsrcs, ja.accumulate, ja.bns = \
        C.addressof(vs0), 1, C.addressof(vd0), 0.1, dd0.data_ptr(), C.addressof(dsa), C.addressof(aa), C.addressof(bpa)
    jb.srcs, jb.nsrc, jb.dst, jb.out_slope, jb.ddst, jb.dst_dpool, jb.dsrcs, jb.accumulate = \
        C.addressof(vs1), 1, C.addressof(vd1), 1.0, dd1.data_ptr(), (dp1.data_ptr() if dpool else None), C.addressof(dsb), C.addressof(ab)

    def single(j, s):
        bns = C.cast(j.bns, C.POINTER(C.c_void_p))[0] if j.bns else None
        return L.lhn_ew_bwd3(C.c_void_p(j.srcs), C.c_void_p(j.dst), C.c_void_p(j.ddst), C.c_void_p(j.dst_dpool), C.c_float(j.out_slope),
                             C.c_void_p(C.cast(j.dsrcs, C.POINTER(C.c_void_p))[0]), C.cast(j.accumulate, C.POINTER(C.c_int))[0],
                             C.c_void_p(bns), s)
    rc = _call(L, pair, L.lhn_ew_bwd_pair, ja, jb, single)
    out = {"dsrc0": _np(ds0), "dsrc1": _np(ds1), "sums0": _np(sums0)}
    out.update({"ref.g": out["dsrc0"][..., 8:16], "ref.raw": _np(s0)[..., 8:16], "ref.table": _np(t0)[:, 8:16], "ref.save": _np(save0),
                "ref.coff": np.int64(4)})
    return rc, out


def _ew_bwd_multi(dev, pair):
    L, c, h, w = _lib.lib(), 8, 4, 4
    d0, dd0 = _t(dev, (N, h, w, 16), 71), _t(dev, (N, h, w, 16), 72)              # the two halves of one destination
    a0, a1, b0, b1 = _t(dev, (N, h, w, 8), 73), _t(dev, (N, h, w, 16), 74), _t(dev, (N, h, w, 8), 75), _t(dev, (N, h, w, 8), 76)
    tb1 = _tab(dev, 8, 77)
    da0, da1, db0, db1 = _t(dev, (N, h, w, 8), 78), _full(dev, (N, h, w, 16)), _t(dev, (N, h, w, 8), 79), _full(dev, (N, h, w, 8))
    sums1, save1, bs1 = _bns(dev, 8, 0, 80)
    sa = (_lib.View * 2)(_view(a0, 0, c), _view(a1, 8, c))
    sb = (_lib.View * 2)(_view(b0, 0, c), _view(b1, 0, c, tb1))
    va, vb = _view(d0, 0, c), _view(d0, 8, c)
    ja, jb = EwJob(), EwJob()
    dsa, dsb = (C.c_void_p * 2)(da0.data_ptr(), da1.data_ptr()), (C.c_void_p * 2)(db0.data_ptr(), db1.data_ptr())
    aa, ab = (C.c_int * 2)(1, 0), (C.c_int * 2)(1, 0)                            # mixed: accumulate into da0 / db0, store da1 / db1
    bpb = (C.c_void_p * 2)(None, C.addressof(bs1))
    ja.srcs, ja.nsrc, ja.dst, ja.out_slope, ja.ddst, ja.dsrcs, ja.accumulate = \
        C.addressof(sa), 2, C.addressof(va), 0.1, dd0.data_ptr(), C.addressof(dsa), C.addressof(aa)
    jb.srcs, jb.nsrc, jb.dst, jb.out_slope, jb.ddst, jb.dsrcs, jb.accumulate, jb.bns = \
        C.addressof(sb), 2, C.addressof(vb), 1.0, dd0.data_ptr(), C.addressof(dsb), C.addressof(ab), C.addressof(bpb)
    single = lambda j, s: L.lhn_ew_bwd_multi(C.c_void_p(j.srcs), j.nsrc, C.c_void_p(j.dst), C.c_void_p(j.ddst), C.c_void_p(j.dst_dpool),      # noqa: E731
                                             C.c_float(j.out_slope), C.c_void_p(j.dsrcs), C.c_void_p(j.accumulate), C.c_void_p(j.bns), s)
    rc = _call(L, pair, L.lhn_ew_bwd_multi_pair, ja, jb, single)
    out = {"da0": _np(da0), "da1": _np(da1), "db0": _np(db0), "db1": _np(db1), "sums1": _np(sums1)}
    out.update({"ref.g": out["db1"], "ref.raw": _np(b1), "ref.table": _np(tb1), "ref.save": _np(save1), "ref.coff": np.int64(0)})
    return rc, out


def _avgpool(dev, pair, c, stat=False):
    L, h, w = _lib.lib(), 16, 24                # 2 x 3 bins of 8 x 8 = 64 pixels: the workgroup kernel
    x0, t0, g0 = _t(dev, (N, h, w, 2 * c), 81), _tab(dev, 2 * c, 82), _gate(dev, 2 * c, 83)
    x1 = _t(dev, (N, h, w, c), 84)
    out = _full(dev, (N, 2, 3, 2 * c))
    pst = _full(dev, (N * 6, 2, c))
    v0, v1 = _view(x0, c, c, t0, g0), _view(x1, 0, c)
    ja, jb = AvgpoolJob(), AvgpoolJob()
    ja.x, ja.out, ja.OH, ja.OW, ja.out_cstride, ja.out_coff = C.addressof(v0), out.data_ptr(), 2, 3, 2 * c, 0
    jb.x, jb.out, jb.OH, jb.OW, jb.out_cstride, jb.out_coff = C.addressof(v1), out.data_ptr(), 2, 3, 2 * c, c
    if stat:
        jb.pstat = pst.data_ptr()
    single = lambda j, s: L.lhn_avgpool_fwd2(C.c_void_p(j.x), C.c_void_p(j.out), j.OH, j.OW, j.out_cstride, j.out_coff, s)      # noqa: E731
    rc = _call(L, pair, L.lhn_avgpool_fwd_pair, ja, jb, single)
    return rc, {"pooled": _np(out), "pstat": _np(pst)}


def _finalize(dev, pair, training):
    L, count = _lib.lib(), 2.0 * 8 * 8
    jobs, keep, outs = [], [], {}
    for k, (c, cs, coff, bias) in enumerate(((8, 24, 4, False), (12, 12, 0, True))):
        rep = torch.arange(REPLICAS, dtype=torch.float64).reshape(REPLICAS, 1)
        mean, var = 0.3 * _rand((c,), 91 + 10 * k).double(), 0.5 + _rand((c,), 92 + 10 * k).double().abs()
        wgt = (1 + rep + 0.01 * torch.arange(c, dtype=torch.float64)) / (1 + rep).sum()      # 32 replicas, every value distinct
        stats = torch.stack([wgt * count * mean, wgt * count * (var + mean * mean)], 1).contiguous().to(dev)      # [32][2][c]
        gamma, beta = (1 + 0.2 * _rand((c,), 93 + 10 * k)).to(dev), (0.1 * _rand((c,), 94 + 10 * k)).to(dev)
        rm, rv = (0.2 * _rand((c,), 95 + 10 * k)).to(dev), (0.7 + _rand((c,), 96 + 10 * k).abs()).to(dev)
        nbt = torch.tensor([3 + 2 * k], dtype=torch.int64, device=dev)
        table, save = _full(dev, (3, cs)), _full(dev, (2, c))
        cb = (0.05 * _rand((c,), 97 + 10 * k)).to(dev) if bias else None
        f = BnFin()
        f.gamma, f.beta, f.running_mean, f.running_var, f.num_batches_tracked = gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), nbt.data_ptr()
        f.table, f.save_mean_invstd, f.count, f.cstride, f.coff, f.C = table.data_ptr(), save.data_ptr(), count, cs, coff, c
        f.eps, f.momentum, f.slope, f.conv_bias = 1e-5, 0.1, 0.1 * k, (cb.data_ptr() if bias else None)
        jobs.append((stats, f))
        keep += [gamma, beta, cb]
        outs[k] = dict(table=table, save=save, rm=rm, rv=rv, nbt=nbt)
    s = _lib.stream()
    (sa, fa), (sb, fb) = jobs
    if pair:
        rc = L.lhn_bn_finalize_pair(_p(sa), C.byref(fa), fa.C, _p(sb), C.byref(fb), fb.C, training, s)
    else:
        rc = 0
        for st, f in jobs:
            rc = rc or L.lhn_bn_finalize2(_p(st), C.c_void_p(f.gamma), C.c_void_p(f.beta), C.c_void_p(f.running_mean), C.c_void_p(f.running_var),
                                          C.c_void_p(f.num_batches_tracked), C.c_void_p(f.table), f.cstride, f.coff, f.C, f.C,
                                          C.c_void_p(f.save_mean_invstd), C.c_double(f.count), C.c_float(f.eps), C.c_float(f.momentum),
                                          C.c_float(f.slope), training, C.c_void_p(f.conv_bias), s)
    return rc, {f"{name}{k}": _np(t) for k, d in outs.items() for name, t in d.items()}


def run(case, dev, pair):
    """(status, every buffer the case may write) of the pair entry (pair=True) or of the two single entries."""
    fn = {"maxpool_fwd": lambda: _maxpool_fwd(dev, pair), "maxpool_bwd_c8": lambda: _maxpool_bwd(dev, pair, 8),
          "maxpool_bwd_c20": lambda: _maxpool_bwd(dev, pair, 20), "ew_fwd": lambda: _ew_fwd(dev, pair),
          "ew_bwd": lambda: _ew_bwd(dev, pair, False), "ew_bwd_dpool": lambda: _ew_bwd(dev, pair, True),
          "ew_bwd_multi": lambda: _ew_bwd_multi(dev, pair), "avgpool_c8": lambda: _avgpool(dev, pair, 8),
          "avgpool_c20": lambda: _avgpool(dev, pair, 20), "finalize_train": lambda: _finalize(dev, pair, 1),
          "finalize_eval": lambda: _finalize(dev, pair, 0),
          # refused by the pair entry (the single calls of the same arguments run)
          "refuse_geometry": lambda: _maxpool_fwd(dev, pair, hb=9), "refuse_overlap": lambda: _maxpool_fwd(dev, pair, overlap=True),
          "refuse_stat_pool": lambda: _avgpool(dev, pair, 8, stat=True), "refuse_bilinear": lambda: _ew_fwd(dev, pair, mode=2)}[case]
    rc, out = fn()
    torch.cuda.synchronize()
    return rc, out


REFUSE = {"refuse_geometry": "differ in geometry", "refuse_overlap": "outputs overlap", "refuse_stat_pool": "statistics / copy forms",
          "refuse_bilinear": "product and bilinear"}


def sums_reference(out, dtype):
    """The BatchNorm-backward sums a job adds, summed over the replicas, from the gradient it stored (ref.g), its raw input and table
    and the producer's saved mean | invstd: [2][C] = sum du | sum du * xhat with du = g * act'(raw * scale + shift)."""
    g, raw = torch.from_numpy(out["ref.g"]).to(dtype), torch.from_numpy(out["ref.raw"]).to(dtype)
    tab, save, coff = torch.from_numpy(out["ref.table"]).to(dtype), torch.from_numpy(out["ref.save"]).to(dtype), int(out["ref.coff"])
    c = g.shape[-1]
    cp = save.numel() // 2
    mean, inv = save[coff:coff + c], save[cp + coff:cp + coff + c]
    u = raw * tab[0] + tab[1]
    du = g * torch.where(u > 0, torch.ones_like(u), tab[2].expand_as(u))
    return torch.stack([du.sum((0, 1, 2)), (du * ((raw - mean) * inv)).sum((0, 1, 2))]).double().numpy()


if __name__ == "__main__":
    dst, names = sys.argv[1], sys.argv[2:] or CASES
    dev = torch.device("cuda:0")
    res = {}
    for nm in names:
        for pair in (True, False):
            rc, out = run(nm, dev, pair)
            assert rc == 0, (nm, pair, rc, _lib.lib().lhn_last_error().decode())
            for k, v in out.items():
                res[f"{nm}/{int(pair)}/{k}"] = v
    np.savez(dst, **res)
