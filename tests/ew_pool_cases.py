"""Cases of the kernels that sit between two convolutions of a plan -- the elementwise combine and its backward forms, the bilinear
backward, channel shuffle, the 2x2 ceil-mode max pool, the adaptive average pool (forward, STAT, COPY, backward) and the gate-gradient
reduce (csrc/k_misc.hip, csrc/k_hrnet.hip) -- run through the C ABI, with a plain torch reference on the CPU (float64, or float32
to measure what the same operation loses in the kernels' own precision).  Imported by tests/test_ew_pool_gpu.py; run as a script
(a child process with its own environment, e.g. LHN_DETERMINISTIC=1) it writes the kernel outputs of the named cases to an .npz file:
    python tests/ew_pool_cases.py OUT.npz REPEATS GROUP:NAME ...
    python tests/ew_pool_cases.py --check-reference   (CPU only: every case's inputs, the input conditions, both references)
    python tests/ew_pool_cases.py --instances         (the table of profiles/ew_pool_instances.md)

Conventions (include/lhn.h): the consumed value of a view is lrelu(raw * scale + shift, slope) * gate[n][c]; every gradient the
backward kernels hand back is the gradient with respect to that consumed value; a leaky output activation's derivative is read
from the sign of the stored dst, SiLU and ReLU-sigmoid derivatives are recomputed from the source's value."""
import ctypes as C
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pw_cases import PREFILL, BnSum, _lib, _outside, _rand, rel_err  # noqa: E402,F401
from litehandnet_amd._lib import View  # noqa: E402

SILU, RSIG = 2.0, 3.0            # LHN_SLOPE_SILU, LHN_SLOPE_RELU_SIGMOID
REPLICAS = 32                    # LHN_STAT_REPLICAS
PAD = 64                         # floats (doubles) behind every output buffer: must keep their prefill
MARGIN = 1e-3                    # input condition: a value whose sign picks a branch is 0 or at least this far (relative) from 0


class GradAdds(C.Structure):     # lhn_grad_adds (include/lhn.h)
    _fields_ = [("same", C.c_void_p), ("same_cstride", C.c_int32), ("same_coff", C.c_int32), ("pooled", C.c_void_p),
                ("OH", C.c_int32), ("OW", C.c_int32), ("pooled_cstride", C.c_int32), ("pooled_coff", C.c_int32)]


class BnSlices(C.Structure):     # lhn_bn_slices (include/lhn.h)
    _fields_ = [("save", C.c_void_p * 2), ("sums", C.c_void_p * 2), ("lo", C.c_int32 * 2), ("C", C.c_int32 * 2), ("n", C.c_int32)]


def V(h, w, cs=None, coff=0, tab=False, gate=False, slope=0.1):
    """A view: h x w pixels, channels [coff, coff + c) of a buffer of cs channels (default: the whole buffer), pending table, gate."""
    return dict(h=h, w=w, cs=cs, coff=coff, tab=tab, gate=gate, slope=slope)


def S(v, acc=0, bns=False, skip=False):
    return dict(v=v, acc=acc, bns=bns, skip=skip)


# ---------------------------------------------------------------- case tables
# thread layout of every kernel here: C4 = C / 4 channel groups, PL = 256 / C4 pixel lanes; the plain combine takes 4 * PL pixels per pass
EWF = {      # lhn_ew_fwd3
    "pass2_tail": dict(n=2, c=128, srcs=[V(5, 37, 192, 64, tab=True, gate=True)], dst=V(5, 37, 168, 32), slope=0.1),   # PL = 8: 32 + 5 pixels
    "nearest3": dict(n=2, c=32, srcs=[V(12, 20, tab=True), V(6, 10, 40, 8, tab=True), V(3, 5, gate=True)], dst=V(12, 20), slope=0.0),
    "float_rule_c20": dict(n=2, c=20, srcs=[V(3, 6, 24, 4, tab=True)], dst=V(7, 74, 28, 8), slope=1.0),   # 6 -> 74: float32 index rule; C4 = 5
    "ratio_14_46": dict(n=1, c=8, srcs=[V(5, 46), V(5, 14, tab=True)], dst=V(5, 46), slope=0.25),        # 14 -> 46: the other such pair
    "coef_c4": dict(n=2, c=4, srcs=[V(6, 9, 8, 4, tab=True), V(3, 3, tab=True)], dst=V(6, 9), slope=0.1, coef=(0.5, -2.0)),        # PL = 256
    "coef3": dict(n=1, c=16, srcs=[V(4, 6, tab=True), V(4, 6), V(2, 3, gate=True)], dst=V(4, 6), slope=1.0, coef=(0.5, -2.0, 1.25)),
    "c1024": dict(n=1, c=1024, srcs=[V(2, 6, tab=True)], dst=V(2, 6), slope=0.1),                        # PL = 1
    "silu": dict(n=2, c=32, srcs=[V(5, 7, 40, 4, tab=True, gate=True)], dst=V(5, 7), slope=SILU),
    "relu_sigmoid": dict(n=2, c=40, srcs=[V(5, 7, tab=True)], dst=V(5, 7, 48, 8), slope=RSIG),
    "product": dict(n=2, c=40, srcs=[V(8, 16, tab=True, gate=True), V(2, 4, 48, 4, tab=True, gate=True)], dst=V(8, 16, 48, 4), slope=1.0, mode=1),
    "bilinear": dict(n=3, c=40, srcs=[V(8, 10), V(4, 5, 48, 8, tab=True, gate=True)], dst=V(8, 10, 44, 4), slope=0.01, mode=2),
    "bilinear_axis1": dict(n=2, c=16, srcs=[V(4, 9, tab=True), V(1, 3, tab=True)], dst=V(4, 9), slope=1.0, mode=2),
    "bilinear_3to7": dict(n=1, c=8, srcs=[V(7, 11), V(3, 4, tab=True)], dst=V(7, 11), slope=0.1, mode=2),   # non-integer ratios 2/6, 3/10
    "product_bilinear": dict(n=2, c=24, srcs=[V(6, 8, tab=True), V(3, 3, tab=True, gate=True)], dst=V(6, 8), slope=1.0, mode=3),
    "det_rows": dict(n=3, c=40, srcs=[V(8, 21, tab=True, gate=True), V(4, 7, tab=True)], dst=V(8, 21, 48, 8), slope=0.1),
}
EWB = {      # lhn_ew_bwd3 / lhn_ew_bwd_multi / lhn_ew_bwd
    "same_leaky": dict(n=2, c=32, dst=V(5, 7, 40, 8), slope=0.01, srcs=[S(V(5, 7, 48, 4))]),
    "same_relu_acc": dict(n=2, c=32, dst=V(5, 7), slope=0.0, srcs=[S(V(5, 7), acc=1)]),
    "same_identity": dict(n=2, c=20, dst=V(5, 7, 24, 4), slope=1.0, srcs=[S(V(5, 7, 28, 8))]),
    "fan2x2_gate": dict(n=2, c=32, dst=V(6, 10, 40, 4, gate=True), slope=0.01, srcs=[S(V(3, 5), acc=1)]),
    "fan4x4": dict(n=2, c=16, dst=V(8, 12), slope=0.1, srcs=[S(V(2, 3, 24, 8))]),
    "fan2x3": dict(n=1, c=40, dst=V(4, 9), slope=1.0, srcs=[S(V(2, 3))]),
    "dpool_7x9": dict(n=3, c=32, dst=V(7, 9, 48, 8, gate=True), dpool=True, slope=0.01, srcs=[S(V(7, 9, 40, 4), acc=1)]),
    "dpool_fan2": dict(n=2, c=16, dst=V(14, 10, gate=True), dpool=True, slope=0.1, srcs=[S(V(7, 5))]),
    "bns_c32": dict(n=3, c=32, dst=V(7, 9), slope=0.01, srcs=[S(V(7, 9, tab=True), bns=True)]),                 # atomics path of lhn_bns_flush
    "bns_c40_fan2": dict(n=2, c=40, dst=V(6, 10, 48, 4), slope=0.1, srcs=[S(V(3, 5, 48, 8, tab=True), acc=1, bns=True)]),   # LDS path
    "silu": dict(n=2, c=32, dst=V(5, 7, gate=True), slope=SILU, srcs=[S(V(5, 7, 40, 8, tab=True, gate=True))]),
    "relu_sigmoid": dict(n=2, c=40, dst=V(5, 7, 48, 4), dpool=True, slope=RSIG, srcs=[S(V(5, 7, tab=True, gate=True), acc=1)]),
    "multi2": dict(n=3, c=32, api="multi", dst=V(7, 9, 40, 8, gate=True), dpool=True, slope=0.01,
                   srcs=[S(V(7, 9, 40, 4, tab=True), bns=True), S(V(7, 9), acc=1)]),
    "multi3": dict(n=2, c=40, api="multi", dst=V(5, 6), slope=0.0,
                   srcs=[S(V(5, 6), acc=1), S(V(5, 6, 48, 8, tab=True), bns=True), S(V(5, 6, 44, 4, tab=True), acc=1, bns=True)]),
    "multi2_identity": dict(n=1, c=16, api="multi", dst=V(3, 4), slope=1.0, srcs=[S(V(3, 4)), S(V(3, 4, 24, 4), acc=1)]),
    "list_skip": dict(n=2, c=32, api="list", dst=V(6, 8, 40, 4, gate=True), slope=0.1,
                      srcs=[S(V(6, 8, 36, 4), acc=1), S(V(6, 8), skip=True), S(V(3, 4))]),
}
MUL = {      # lhn_ew_mul_bwd, both operands of the product (EWF["product"]): d_x reads the small operand, d_g sums its fan-out
    "product": dict(n=2, c=40, x=V(8, 16, tab=True, gate=True), g=V(2, 4, 48, 4, tab=True, gate=True), dst=V(8, 16, 48, 4), acc=(0, 1)),
    "product_det": dict(n=3, c=16, x=V(12, 6, 24, 8, tab=True, gate=True), g=V(6, 3, tab=True, gate=True), dst=V(12, 6), acc=(1, 0)),
}
BIL = {      # lhn_bilinear_bwd: dst = lrelu(a + bilinear(b)), the gradient of b
    "4x5_leaky": dict(n=2, c=40, a=V(8, 10), b=V(4, 5, 48, 8, tab=True, gate=True), dst=V(8, 10, 44, 4), slope=0.01, acc=0),
    "4x5_identity_acc": dict(n=2, c=40, a=V(8, 10), b=V(4, 5, 48, 8, tab=True, gate=True), dst=V(8, 10, 44, 4), slope=1.0, acc=1),
    "axis1_leaky_acc": dict(n=2, c=16, a=V(4, 9), b=V(1, 3, tab=True), dst=V(4, 9), slope=0.01, acc=1),
    "3x4_to_7x11": dict(n=1, c=8, a=V(7, 11), b=V(3, 4, tab=True), dst=V(7, 11), slope=1.0, acc=0),
    "det_rows": dict(n=5, c=20, a=V(9, 7), b=V(4, 3, 24, 4, tab=True), dst=V(9, 7), slope=0.01, acc=0),
}
SHF = {      # lhn_shuffle2_fwd (c = channels of each input; dst has 2 * c)
    "tables_gates": dict(n=2, c=20, h=5, w=7, a=V(5, 7, 32, 8, tab=True, gate=True), b=V(5, 7, 28, 4, tab=True, gate=True), dst=V(5, 7, 48, 4)),
    "plain_move": dict(n=3, c=16, h=6, w=9, a=V(6, 9, 24, 4), b=V(6, 9, 20, 4), dst=V(6, 9, 40, 8), exact=("dst",)),
}
SHB = {      # lhn_shuffle2_bwd
    "da_store": dict(n=2, c=20, a=V(5, 7, 32, 8), b=V(5, 7, 28, 4), dst=V(5, 7, 48, 4), which="a", acc=(0, 0)),
    "db_acc": dict(n=2, c=20, a=V(5, 7, 32, 8), b=V(5, 7, 28, 4), dst=V(5, 7, 48, 4), which="b", acc=(0, 1)),
    "both_mixed": dict(n=3, c=16, a=V(6, 9, 24, 4), b=V(6, 9, 20, 4), dst=V(6, 9, 40, 8), which="ab", acc=(1, 0)),
    "both_acc": dict(n=3, c=16, a=V(6, 9, 24, 4), b=V(6, 9, 20, 4), dst=V(6, 9), which="ab", acc=(1, 1)),
}
MP = {       # lhn_maxpool2_fwd + lhn_maxpool2_bwd3 (inputs on a power-of-two grid: exact ties, see _make)
    "8x12": dict(n=2, c=32, x=V(8, 12, 40, 4, tab=True, gate=True, slope=0.25), y=V(4, 6, 48, 8), acc=0),
    "7x9_ties0": dict(n=5, c=32, x=V(7, 9, 40, 4, tab=True, slope=0.0), y=V(4, 5), acc=1, bns=True),       # whole windows tie at exactly 0
    "7x9_c20": dict(n=2, c=20, x=V(7, 9, tab=True, slope=0.0), y=V(4, 5, 24, 4), acc=0, bns=True),         # LDS path of the sums
    "1x1": dict(n=3, c=16, x=V(1, 1, tab=True, slope=0.25), y=V(1, 1), acc=0),
    "adds_same": dict(n=2, c=32, x=V(8, 8, 40, 8, tab=True, slope=0.0), y=V(4, 4), acc=0, same=(48, 12)),
    "adds_pooled3": dict(n=2, c=32, x=V(8, 8, tab=True, gate=True, slope=0.25), y=V(4, 4), acc=1, pooled=(3, 3, 40, 4)),      # overlapping bins
    "adds_both": dict(n=2, c=16, x=V(8, 12, 24, 4, tab=True, slope=0.0), y=V(4, 6), acc=0, same=(16, 0), pooled=(3, 3, 16, 0)),
}
APF = {      # lhn_avgpool_fwd2 / lhn_avgpool_fwd4
    "small_8to4": dict(n=2, c=32, x=V(8, 8, 40, 4, tab=True), OH=4, OW=4),
    "small_7to3_gate": dict(n=2, c=20, x=V(7, 7, tab=True, gate=True), OH=3, OW=3, ocs=32, ocoff=8),
    "wg_16x24_c64": dict(n=2, c=64, x=V(16, 24, 72, 4, tab=True), OH=3, OW=3),
    "wg_17x23_1x1": dict(n=2, c=64, x=V(17, 23, tab=True, gate=True), OH=1, OW=1, ocs=96, ocoff=16),       # 391 pixels: unrolled loop + tail
    "wg_c20": dict(n=2, c=20, x=V(16, 24, 24, 4, tab=True), OH=3, OW=3),                                    # LDS reduction, C4 = 5
    "wg_c40": dict(n=1, c=40, x=V(17, 23, tab=True, gate=True), OH=3, OW=3),
    "wg_c512": dict(n=1, c=512, x=V(11, 13, tab=True), OH=1, OW=1),                                         # C4 = 128 > 64, PL = 2
    "wg_c4": dict(n=2, c=4, x=V(17, 23, 8, 4, tab=True), OH=3, OW=3),                                       # PL = 256
    "stat": dict(n=2, c=64, x=V(16, 24, tab=True), OH=3, OW=3, stat=[(16, 16), (32, 32)]),                  # channels [0, 16): pass-through
    "stat_c40": dict(n=2, c=40, x=V(17, 23, tab=True), OH=3, OW=3, stat=[(8, 32)]),
    "copy": dict(n=2, c=64, x=V(16, 24, tab=True), OH=3, OW=3, copy=V(16, 24, 40, 4, tab=True, gate=True), copy_c=32),
    "stat_copy": dict(n=2, c=40, x=V(17, 23, tab=True), OH=3, OW=3, stat=[(20, 20)], copy=V(17, 23, 24, 4, tab=True, gate=True), copy_c=20),
}
APB = {      # lhn_avgpool_bwd3
    "8to4": dict(n=2, c=32, x=V(8, 8, 40, 4), OH=4, OW=4, acc=0),
    "7to3_acc": dict(n=2, c=20, x=V(7, 7), OH=3, OW=3, ocs=32, ocoff=8, acc=1),
    "16x24_to3_bns": dict(n=2, c=64, x=V(16, 24, 72, 4, tab=True), OH=3, OW=3, acc=0, bns=True),
    "17x23_to1": dict(n=2, c=64, x=V(17, 23), OH=1, OW=1, ocs=96, ocoff=16, acc=1),
    "c40_bns_acc": dict(n=2, c=40, x=V(17, 23, tab=True), OH=3, OW=3, acc=1, bns=True),                      # LDS path of the sums
    "full_size": dict(n=1, c=16, x=V(5, 6), OH=5, OW=6, acc=0),                                            # OH = H: every bin is one pixel
}
GATE = {     # lhn_gate_bwd_reduce3
    "slice_no_tsum": dict(n=2, c=32, y=V(9, 11, 48, 8, tab=True, gate=True), pre=1),
    "tsum_two_slices": dict(n=2, c=64, y=V(9, 11, tab=True), tsum=True, stat=[(0, 32), (48, 16)], pre=1),
    "hw1": dict(n=3, c=20, y=V(1, 1, tab=True), tsum=True, stat=[(0, 20)], pre=1),
    "hw130": dict(n=2, c=64, y=V(10, 13, tab=True), tsum=True, stat=[(0, 64)], pre=1),                      # two chunks of 65: duplicated last pixel
    "64x64": dict(n=2, c=32, y=V(64, 64, tab=True), tsum=True, stat=[(0, 16), (16, 16)], pre=1),            # 32 chunks
    "garbage_not_prezeroed": dict(n=2, c=40, y=V(9, 11, tab=True), tsum=True, stat=[(0, 40)], pre=0),
}
GROUPS = {"ewf": EWF, "ewb": EWB, "mul": MUL, "bil": BIL, "shf": SHF, "shb": SHB, "mp": MP, "apf": APF, "apb": APB, "gate": GATE}
# LHN_DETERMINISTIC=1: 2 CUs are reported, the row grids cap at 16 workgroups -- cases whose row count is larger (rows())
DET = ["ewf:nearest3", "ewf:det_rows", "ewf:bilinear", "ewb:dpool_7x9", "ewb:bns_c32", "ewb:multi2", "mul:product_det", "bil:det_rows",
       "shf:plain_move", "shb:both_mixed", "mp:7x9_ties0", "apb:16x24_to3_bns", "apb:c40_bns_acc", "gate:64x64"]


def rows(group, name):
    """Rows (or work items) the kernel's grid-stride loop runs over."""
    c = GROUPS[group][name]
    n = c["n"]
    if group in ("ewf", "shf", "shb"):
        return n * c["dst"]["h"]
    if group == "ewb":
        return n * min(s["v"]["h"] for s in c["srcs"] if not s["skip"])
    if group == "mul":
        return n * c["g"]["h"]
    if group == "bil":
        return n * c["b"]["h"]
    if group == "mp":
        return n * c["y"]["h"]
    if group == "apb":
        return n * c["x"]["h"]
    if group == "gate":
        return c["y"]["h"] * c["y"]["w"] // 128           # chunks of a split launch; one workgroup per image when deterministic
    return n * c["OH"] * c["OW"]


# ---------------------------------------------------------------- inputs
def _tab(cs, seed, slope):
    sign = torch.where(torch.arange(cs) % 3 == 1, -1.0, 1.0)
    return torch.stack([sign * (0.6 + 0.4 * _rand((cs,), seed).abs()), 0.2 * _rand((cs,), seed + 1), torch.full((cs,), float(slope))]).contiguous()


def _away(t):
    """Move every element closer to 0 than 4 * MARGIN of the largest magnitude out to that distance (its sign picks a branch)."""
    lim = 4 * MARGIN * float(t.abs().max())
    return torch.where(t.abs() < lim, torch.where(t >= 0, lim, -lim).to(t.dtype), t)


def _make(g, key, n, c, v, seed, grid=False):
    """Raw buffer, table and gate of a view.  With a table the raw values are nudged until no raw * scale + shift lies within
    MARGIN of 0.  grid: everything on a power-of-two grid (raw in quarters, scale in {1, 2, -1, 0.5}, shift in quarters, gate in
    quarters): float32 and float64 then agree in every bit, equal values tie exactly and unequal ones differ by at least 1/64."""
    cs = v["cs"] or c
    if grid:
        rng = np.random.Generator(np.random.PCG64(seed))
        g[key] = torch.from_numpy((rng.integers(-8, 9, (n, v["h"], v["w"], cs)) / 4).astype(np.float32))
        if v["tab"]:
            g[key + "_tab"] = torch.stack([torch.tensor([1.0, 2.0, -1.0, 0.5])[torch.from_numpy(rng.integers(0, 4, cs))],
                                           torch.from_numpy((rng.integers(-2, 3, cs) / 4).astype(np.float32)), torch.full((cs,), float(v["slope"]))]).contiguous()
        if v["gate"]:
            g[key + "_gate"] = torch.from_numpy((rng.integers(2, 7, (n, cs)) / 4).astype(np.float32))
        return
    raw = _rand((n, v["h"], v["w"], cs), seed)
    if v["tab"]:
        tab = g[key + "_tab"] = _tab(cs, seed + 1, v["slope"])
        u = raw * tab[0] + tab[1]
        lim = 4 * MARGIN * float(u.abs().max())
        raw = torch.where(u.abs() < lim, raw + 3 * lim / tab[0], raw)
        g.setdefault("_kinks", []).append(key)
    if v["gate"]:
        g[key + "_gate"] = torch.sigmoid(_rand((n, cs), seed + 3))
    g[key] = raw.contiguous()


def _sl(c, v):
    return slice(v["coff"], v["coff"] + c)


def _val(g, key, c, v, dt, gate=True):
    """Consumed value of the view's channels, [N, H, W, C]."""
    s = _sl(c, v)
    x = g[key][..., s].to(dt)
    if v["tab"]:
        t = g[key + "_tab"][:, s].to(dt)
        u = x * t[0] + t[1]
        x = torch.where(u > 0, u, u * t[2])
    if v["gate"] and gate:
        x = x * g[key + "_gate"][:, s].to(dt)[:, None, None, :]
    return x


def _dact(g, key, c, v, dt):
    s = _sl(c, v)
    t = g[key + "_tab"][:, s].to(dt)
    u = g[key][..., s].to(dt) * t[0] + t[1]
    return torch.where(u > 0, torch.ones_like(u), t[2].expand_as(u))


def _save(g, key, ch, seed):
    g[key] = torch.stack([0.1 * _rand((ch,), seed), 1 + 0.2 * _rand((ch,), seed + 1).abs()]).contiguous()


BNS_EXTRA, BNS_COFF = 16, 8      # a reader's view starts at channel 8 of a producer BatchNorm that is 16 channels wider


def _bins(size, out):
    return [((i * size) // out, -((-(i + 1) * size) // out)) for i in range(out)]


def _dpool25(d9):
    """lhn_dpool_store: segment s of an axis lies in bin b iff s in {2b - 1, 2b, 2b + 1}; [N, 9, C] -> [N, 25, C]."""
    out = torch.zeros(d9.shape[0], 25, d9.shape[2])
    for sh in range(5):
        for sw in range(5):
            for bi in range(3):
                for bj in range(3):
                    if abs(sh - 2 * bi) <= 1 and abs(sw - 2 * bj) <= 1:
                        out[:, sh * 5 + sw] += d9[:, bi * 3 + bj]
    return out.contiguous()


def inputs(group, name, seed=7):
    c = GROUPS[group][name]
    n, ch = c["n"], c["c"]
    g = {"seed": seed}
    if group == "ewf":
        for i, v in enumerate(c["srcs"]):
            _make(g, f"s{i}", n, ch, v, seed + 10 * i)
    elif group == "ewb":
        d = c["dst"]
        dcs = d["cs"] or ch
        g["dst"] = _away(_rand((n, d["h"], d["w"], dcs), seed))
        g["_signs"] = ["dst"]
        g["ddst"] = _rand((n, d["h"], d["w"], dcs), seed + 1)
        if d["gate"]:
            g["dst_gate"] = torch.sigmoid(_rand((n, dcs), seed + 2))
        if c.get("dpool"):
            g["d9"] = 0.3 * _rand((n, 9, dcs), seed + 3)
            g["dpool"] = _dpool25(g["d9"])
        for i, s in enumerate(c["srcs"]):
            v = s["v"]
            _make(g, f"s{i}", n, ch, v, seed + 10 * (i + 1))
            g[f"prior{i}"] = _rand((n, v["h"], v["w"], v["cs"] or ch), seed + 10 * (i + 1) + 5)
            if s["bns"]:
                _save(g, f"save{i}", ch + BNS_EXTRA, seed + 10 * (i + 1) + 6)
    elif group == "mul":
        d = c["dst"]
        _make(g, "x", n, ch, c["x"], seed)
        _make(g, "g", n, ch, c["g"], seed + 10)
        g["ddst"] = _rand((n, d["h"], d["w"], d["cs"] or ch), seed + 20)
        g["prior_x"] = _rand(g["x"].shape, seed + 21)
        g["prior_g"] = _rand(g["g"].shape, seed + 22)
    elif group == "bil":
        d = c["dst"]
        _make(g, "a", n, ch, c["a"], seed)
        _make(g, "b", n, ch, c["b"], seed + 10)
        assert not c["a"]["tab"] and not c["a"]["gate"]
        pre = _bil_pre(c, g, torch.float32)          # nudge a until the pre-activation keeps MARGIN from 0
        lim = 4 * MARGIN * float(pre.abs().max())
        g["a"][..., _sl(ch, c["a"])] += torch.where(pre.abs() < lim, 3 * lim, 0.0)
        pre = _bil_pre(c, g, torch.float32)
        g["dst"] = _rand((n, d["h"], d["w"], d["cs"] or ch), seed + 20)
        g["dst"][..., _sl(ch, d)] = F.leaky_relu(pre, c["slope"])        # the stored output of the forward
        g["ddst"] = _rand(g["dst"].shape, seed + 21)
        g["prior"] = _rand(g["b"].shape, seed + 22)
    elif group == "shf":
        _make(g, "a", n, ch, c["a"], seed)
        _make(g, "b", n, ch, c["b"], seed + 10)
    elif group == "shb":
        d = c["dst"]
        g["ddst"] = _rand((n, d["h"], d["w"], d["cs"] or 2 * ch), seed)
        g["prior_a"] = _rand((n, d["h"], d["w"], c["a"]["cs"] or ch), seed + 1)
        g["prior_b"] = _rand((n, d["h"], d["w"], c["b"]["cs"] or ch), seed + 2)
    elif group == "mp":
        x, y = c["x"], c["y"]
        _make(g, "x", n, ch, x, seed, grid=True)
        g["dy"] = _rand((n, y["h"], y["w"], y["cs"] or ch), seed + 1)
        g["prior"] = _rand(g["x"].shape, seed + 2)
        if c.get("bns"):
            _save(g, "save", ch + BNS_EXTRA, seed + 3)
        if c.get("same"):
            g["same"] = _rand((n, x["h"], x["w"], c["same"][0]), seed + 4)
        if c.get("pooled"):
            g["pooled"] = _rand((n, c["pooled"][0], c["pooled"][1], c["pooled"][2]), seed + 5)
    elif group == "apf":
        _make(g, "x", n, ch, c["x"], seed)
        if c.get("copy"):
            _make(g, "src", n, c["copy_c"], c["copy"], seed + 10)
        for k, (lo, cc) in enumerate(c.get("stat", [])):
            _save(g, f"save{k}", cc, seed + 20 + 2 * k)
    elif group == "apb":
        x = c["x"]
        _make(g, "x", n, ch, x, seed)
        g["dout"] = _rand((n, c["OH"], c["OW"], c.get("ocs", ch)), seed + 1)
        g["prior"] = _rand(g["x"].shape, seed + 2)
        if c.get("bns"):
            _save(g, "save", ch + BNS_EXTRA, seed + 3)
    elif group == "gate":
        _make(g, "y", n, ch, c["y"], seed)
        g["dz"] = _rand(g["y"].shape, seed + 1)
        for k, (lo, cc) in enumerate(c.get("stat", [])):
            _save(g, f"save{k}", cc, seed + 20 + 2 * k)
    return g


# ---------------------------------------------------------------- reference (plain torch on the CPU)
def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _act(v, slope):
    if slope == SILU:
        return F.silu(v)
    if slope == RSIG:
        return torch.sigmoid(torch.relu(v))
    return F.leaky_relu(v, slope)


def _resample(v, H, W, bilinear):
    """[N, h, w, C] -> [N, H, W, C]: torch's nearest (float32 index rule in every dtype) or bilinear with align_corners=True."""
    if v.shape[1:3] == (H, W):
        return v
    if bilinear:
        return _nhwc(F.interpolate(_nchw(v), size=(H, W), mode="bilinear", align_corners=True))
    return _nhwc(F.interpolate(_nchw(v), size=(H, W), mode="nearest"))


def _bil_pre(c, g, dt, vb=None):
    vb = _val(g, "b", c["c"], c["b"], dt) if vb is None else vb
    return _val(g, "a", c["c"], c["a"], dt) + _resample(vb, c["dst"]["h"], c["dst"]["w"], True)


def _np(t):
    return t.detach().double().numpy()


def _bnsums(gv, g, key, savekey, c, v, dt):
    """sum du | sum du * xhat of a reader's own contribution gv (gradient of the consumed value, before any accumulate)."""
    du = gv * _dact(g, key, c, v, dt)
    sv = g[savekey][:, BNS_COFF:BNS_COFF + c].to(dt)
    xhat = (g[key][..., _sl(c, v)].to(dt) - sv[0]) * sv[1]
    return _np(du.sum((0, 1, 2))), _np((du * xhat).sum((0, 1, 2)))


def _slice_stats(c, ch, g, dt):
    """mean | invstd per channel of a buffer by the lhn_bn_slices rule: channels outside every slice use 0 and 1."""
    mean, inv = torch.zeros(ch, dtype=dt), torch.ones(ch, dtype=dt)
    for k, (lo, cc) in enumerate(c.get("stat", [])):
        mean[lo:lo + cc], inv[lo:lo + cc] = g[f"save{k}"][0].to(dt), g[f"save{k}"][1].to(dt)
    return mean, inv


def reference(group, name, g=None, dtype=torch.float64):
    c = GROUPS[group][name]
    g = g or inputs(group, name)
    n, ch, dt = c["n"], c["c"], dtype
    out = {}
    if group == "ewf":
        d, mode = c["dst"], c.get("mode", 0)
        coef = c.get("coef") or (1.0,) * len(c["srcs"])
        acc = None
        for i, v in enumerate(c["srcs"]):
            t = _resample(_val(g, f"s{i}", ch, v, dt), d["h"], d["w"], bool(mode & 2)) * coef[i]
            acc = t if acc is None else (acc * t if mode & 1 else acc + t)
        out["dst"] = _np(_act(acc, c["slope"]))
    elif group == "ewb":
        d = c["dst"]
        ds = _sl(ch, d)
        e = g["ddst"][..., ds].to(dt)
        if d["gate"]:
            e = e * g["dst_gate"][:, ds].to(dt)[:, None, None, :]
        if c.get("dpool") and c.get("api") != "list":
            # the pooled gradient of a pixel: the sum over the 3x3 adaptive bins that contain it (the 25 segments are the kernels' layout)
            mh = torch.tensor([[float(lo <= h < hi) for lo, hi in _bins(d["h"], 3)] for h in range(d["h"])], dtype=dt)
            mw = torch.tensor([[float(lo <= w < hi) for lo, hi in _bins(d["w"], 3)] for w in range(d["w"])], dtype=dt)
            e = e + torch.einsum("hi,wj,nijc->nhwc", mh, mw, g["d9"][..., ds].to(dt).view(n, 3, 3, ch))
        if c["slope"] not in (SILU, RSIG) and c["slope"] != 1.0:
            e = e * torch.where(g["dst"][..., ds] > 0, 1.0, c["slope"]).to(dt)
        for i, s in enumerate(c["srcs"]):
            if s["skip"]:
                continue
            v = s["v"]
            leaf = _val(g, f"s{i}", ch, v, dt).clone().requires_grad_(True)
            y = _resample(leaf, d["h"], d["w"], False)
            if c["slope"] in (SILU, RSIG):
                y = _act(y, c["slope"])
            gv, = torch.autograd.grad(y, leaf, e)
            out[f"d{i}"] = _np(gv + g[f"prior{i}"][..., _sl(ch, v)].to(dt) if s["acc"] else gv)
            if s["bns"]:
                out[f"sums_du{i}"], out[f"sums_duxhat{i}"] = _bnsums(gv, g, f"s{i}", f"save{i}", ch, v, dt)
    elif group == "mul":
        d = c["dst"]
        vx = _val(g, "x", ch, c["x"], dt).clone().requires_grad_(True)
        vg = _val(g, "g", ch, c["g"], dt).clone().requires_grad_(True)
        y = vx * _resample(vg, d["h"], d["w"], False)                # the forward graph of EWF["product"]
        gx, gg = torch.autograd.grad(y, [vx, vg], g["ddst"][..., _sl(ch, d)].to(dt))
        out["d_x"] = _np(gx + g["prior_x"][..., _sl(ch, c["x"])].to(dt) if c["acc"][0] else gx)
        out["d_g"] = _np(gg + g["prior_g"][..., _sl(ch, c["g"])].to(dt) if c["acc"][1] else gg)
    elif group == "bil":
        vb = _val(g, "b", ch, c["b"], dt).clone().requires_grad_(True)
        y = F.leaky_relu(_bil_pre(c, g, dt, vb), c["slope"])         # the forward graph of EWF["bilinear"]
        gb, = torch.autograd.grad(y, vb, g["ddst"][..., _sl(ch, c["dst"])].to(dt))
        out["d_b"] = _np(gb + g["prior"][..., _sl(ch, c["b"])].to(dt) if c["acc"] else gb)
    elif group == "shf":
        va, vb = _val(g, "a", ch, c["a"], dt), _val(g, "b", ch, c["b"], dt)
        out["dst"] = _np(torch.stack([va, vb], -1).reshape(n, c["h"], c["w"], 2 * ch))      # channel_shuffle(cat(a, b), 2)
    elif group == "shb":
        dd = g["ddst"][..., _sl(2 * ch, c["dst"])].to(dt)
        for j, k in enumerate("ab"):
            if k in c["which"]:
                gk = dd[..., j::2]
                out[f"d_{k}"] = _np(gk + g[f"prior_{k}"][..., _sl(ch, c[k])].to(dt) if c["acc"][j] else gk)
    elif group == "mp":
        x, y = c["x"], c["y"]
        leaf = _nchw(_val(g, "x", ch, x, dt)).clone().requires_grad_(True)
        yy = F.max_pool2d(leaf, 2, 2, ceil_mode=True)
        out["y"] = _np(_nhwc(yy))
        terms, grads = [yy], [_nchw(g["dy"][..., _sl(ch, y)].to(dt))]
        if c.get("pooled"):
            oh, ow, pcs, pcoff = c["pooled"]
            terms.append(F.adaptive_avg_pool2d(leaf, (oh, ow)))
            grads.append(_nchw(g["pooled"][..., pcoff:pcoff + ch].to(dt)))
        gv = _nhwc(torch.autograd.grad(terms, leaf, grads)[0])
        if c.get("same"):
            gv = gv + g["same"][..., c["same"][1]:c["same"][1] + ch].to(dt)
        out["dx"] = _np(gv + g["prior"][..., _sl(ch, x)].to(dt) if c["acc"] else gv)
        if c.get("bns"):
            out["sums_du"], out["sums_duxhat"] = _bnsums(gv, g, "x", "save", ch, x, dt)
    elif group == "apf":
        x = c["x"]
        val = _val(g, "x", ch, x, dt)
        raw, da = g["x"][..., _sl(ch, x)].to(dt), (_dact(g, "x", ch, x, dt) if "stat" in c else None)
        if c.get("copy"):
            cc = c["copy_c"]
            sv = _val(g, "src", cc, c["copy"], dt)
            out["x_copied"] = _np(sv)
            val = torch.cat([sv, val[..., cc:]], -1)
            if "stat" in c:
                raw = torch.cat([g["src"][..., _sl(cc, c["copy"])].to(dt), raw[..., cc:]], -1)
                da = torch.cat([_dact(g, "src", cc, c["copy"], dt), da[..., cc:]], -1)
        out["pooled"] = _np(_nhwc(F.adaptive_avg_pool2d(_nchw(val), (c["OH"], c["OW"]))))
        if "stat" in c:
            mean, inv = _slice_stats(c, ch, g, dt)
            m1 = da * (raw - mean) * inv
            binsum = lambda t: torch.stack([torch.stack([t[:, h0:h1, w0:w1].sum((1, 2)) for w0, w1 in _bins(x["w"], c["OW"])], 1)   # noqa: E731
                                            for h0, h1 in _bins(x["h"], c["OH"])], 1)
            out["M0"], out["M1"] = _np(binsum(da)), _np(binsum(m1))
    elif group == "apb":
        x = c["x"]
        leaf = _nchw(_val(g, "x", ch, x, dt)).clone().requires_grad_(True)
        oc = c.get("ocoff", 0)
        gv, = torch.autograd.grad(F.adaptive_avg_pool2d(leaf, (c["OH"], c["OW"])), leaf, _nchw(g["dout"][..., oc:oc + ch].to(dt)))
        gv = _nhwc(gv)
        out["dx"] = _np(gv + g["prior"][..., _sl(ch, x)].to(dt) if c["acc"] else gv)
        if c.get("bns"):
            out["sums_du"], out["sums_duxhat"] = _bnsums(gv, g, "x", "save", ch, x, dt)
    elif group == "gate":
        y = c["y"]
        dz = g["dz"][..., _sl(ch, y)].to(dt)
        out["dgate"] = _np((dz * _val(g, "y", ch, y, dt, gate=False)).sum((1, 2)))
        if c.get("tsum"):
            mean, inv = _slice_stats(c, ch, g, dt)
            da = dz * _dact(g, "y", ch, y, dt)
            out["T0"], out["T1"] = _np(da.sum((1, 2))), _np((da * (g["y"][..., _sl(ch, y)].to(dt) - mean) * inv).sum((1, 2)))
    return out


def exact_keys(group, name):
    """Outputs that are pure moves (or one float32 addition) of input floats: bit equality with the float32 reference."""
    if group == "shb":
        return ("d_a", "d_b")
    return GROUPS[group][name].get("exact", ())


# ---------------------------------------------------------------- kernels
def _alloc(shape, dev, init=None, dtype=torch.float32):
    """A tensor of `shape` in front of PAD more elements, all PREFILL (or `init`): (flat buffer, view)."""
    cnt = int(np.prod(shape))
    flat = torch.full((cnt + PAD,), PREFILL, device=dev, dtype=dtype)
    if init is not None:
        flat[:cnt] = init.reshape(-1)
    return flat, flat[:cnt].view(shape)


def _kept(flat, t, coff, c, before=None):
    """Channels outside [coff, coff + c) of t and the PAD elements behind it still hold their bits."""
    ref = torch.full_like(t, PREFILL) if before is None else before
    return np.array(bool((flat[t.numel():] == PREFILL).all()) and torch.equal(_outside(t, coff, c), _outside(ref, coff, c)))


def _dv(d, key, c, v, shape=None, t=None):
    vw = View()
    t = d[key] if t is None else t
    vw.data, vw.pend = t.data_ptr(), None
    vw.table = d[key + "_tab"].data_ptr() if v["tab"] else None
    vw.gate = d[key + "_gate"].data_ptr() if v["gate"] else None
    vw.N, vw.H, vw.W, vw.cstride, vw.coff, vw.C = t.shape[0], t.shape[1], t.shape[2], t.shape[3], v["coff"], c
    return vw


class _Sums:
    """lhn_bnsum over a zeroed [32][2][c + BNS_EXTRA] buffer; folded(): the reader's channels, replicas summed."""

    def __init__(self, save, c, dev):
        self.c, self.bc = c, c + BNS_EXTRA
        self.flat = torch.zeros(REPLICAS * 2 * self.bc + PAD, dtype=torch.float64, device=dev)
        self.s = BnSum()
        self.s.sums, self.s.save, self.s.C, self.s.coff = self.flat.data_ptr(), save.data_ptr(), self.bc, BNS_COFF

    def folded(self, out, sfx=""):
        t = self.flat[:REPLICAS * 2 * self.bc].view(REPLICAS, 2, self.bc)
        tot = t.sum(0)[:, BNS_COFF:BNS_COFF + self.c].cpu().numpy()
        out["sums_du" + sfx], out["sums_duxhat" + sfx] = tot[0], tot[1]
        out[f"sums{sfx}_outside_ok"] = np.array(bool((_outside(t, BNS_COFF, self.c) == 0).all()) and bool((self.flat[t.numel():] == 0).all()))

    def untouched(self):
        return bool((self.flat == 0).all())


def _slices(c, d):
    s = BnSlices()
    s.n = len(c.get("stat", []))
    for k, (lo, cc) in enumerate(c.get("stat", [])):
        s.save[k], s.sums[k], s.lo[k], s.C[k] = d[f"save{k}"].data_ptr(), None, lo, cc
    return s


def run(group, name, dev, g=None, expect_fail=False, case=None):
    """Outputs as numpy arrays (the views' channels) plus `*_ok` flags: every float outside the outputs keeps its bits.
    expect_fail: (status, nothing was written) of a call the library must refuse (`case`: the refused variant)."""
    c = case or GROUPS[group][name]
    g = g or inputs(group, name)
    d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in g.items()}
    L, st = _lib.lib(), _lib.stream()
    n, ch = c["n"], c["c"]
    out, wrote = {}, []          # wrote: (flat, fill) of every buffer a refused call must leave alone
    p, fl = _lib.ptr, C.c_float

    def outbuf(shape, init=None):
        flat, t = _alloc(shape, dev, init)
        wrote.append((flat.clone(), flat))
        return flat, t

    if group == "ewf":
        dv = c["dst"]
        yf, y = outbuf((n, dv["h"], dv["w"], dv["cs"] or ch))
        ns = len(c["srcs"])
        views = (View * ns)(*[_dv(d, f"s{i}", ch, v) for i, v in enumerate(c["srcs"])])
        coef = (fl * ns)(*c["coef"]) if c.get("coef") else None
        rc = L.lhn_ew_fwd3(views, ns, coef, C.byref(_dv(d, None, ch, dv, t=y)), fl(c["slope"]), c.get("mode", 0), st)
        fin = lambda: out.update(dst=y[..., _sl(ch, dv)].cpu().numpy(), dst_outside_ok=_kept(yf, y, dv["coff"], ch))      # noqa: E731
    elif group == "ewb":
        dv, api = c["dst"], c.get("api", "bwd3")
        dview = View()
        dview.data, dview.table, dview.pend = d["dst"].data_ptr(), None, None
        dview.gate = d["dst_gate"].data_ptr() if dv["gate"] else None
        dview.N, dview.H, dview.W, dview.cstride, dview.coff, dview.C = n, dv["h"], dv["w"], d["dst"].shape[3], dv["coff"], ch
        ns = len(c["srcs"])
        bufs, sums = [], []
        for i, s in enumerate(c["srcs"]):
            bufs.append(None if s["skip"] else outbuf(d[f"prior{i}"].shape, d[f"prior{i}"] if s["acc"] else None))
            sums.append(_Sums(d[f"save{i}"], ch, dev) if s["bns"] else None)
        views = (View * ns)(*[_dv(d, f"s{i}", ch, s["v"]) for i, s in enumerate(c["srcs"])])
        dptr = (C.c_void_p * ns)(*[(b[1].data_ptr() if b else None) for b in bufs])
        accs = (C.c_int * ns)(*[s["acc"] for s in c["srcs"]])
        dpool = p(d.get("dpool"))
        if api == "bwd3":
            rc = L.lhn_ew_bwd3(C.byref(views[0]), C.byref(dview), p(d["ddst"]), dpool, fl(c["slope"]), p(bufs[0][1]), c["srcs"][0]["acc"],
                               C.byref(sums[0].s) if sums[0] else None, st)
        elif api == "multi":
            bp = (C.POINTER(BnSum) * ns)(*[(C.pointer(s.s) if s else None) for s in sums])
            rc = L.lhn_ew_bwd_multi(views, ns, C.byref(dview), p(d["ddst"]), dpool, fl(c["slope"]), dptr, accs, bp, st)
        else:
            rc = L.lhn_ew_bwd(views, ns, C.byref(dview), p(d["ddst"]), fl(c["slope"]), dptr, accs, st)

        def fin():
            for i, s in enumerate(c["srcs"]):
                if s["skip"]:
                    continue
                v = s["v"]
                out[f"d{i}"] = bufs[i][1][..., _sl(ch, v)].cpu().numpy()
                out[f"d{i}_outside_ok"] = _kept(bufs[i][0], bufs[i][1], v["coff"], ch, d[f"prior{i}"] if s["acc"] else None)
                if sums[i]:
                    sums[i].folded(out, str(i))
        wrote += [(torch.zeros_like(s.flat), s.flat) for s in sums if s]
    elif group == "mul":
        dv = c["dst"]
        dview = _dv(d, None, ch, dv, t=d["ddst"])        # (the kernel reads only the geometry of dst)
        res = {}
        rc = 0
        for k, o in ((("g", "x"),) if expect_fail else (("x", "g"), ("g", "x"))):      # (the refused variant: the small operand's call)
            j = "xg".index(k)
            res[k] = outbuf(d[f"prior_{k}"].shape, d[f"prior_{k}"] if c["acc"][j] else None)
            rc = rc or L.lhn_ew_mul_bwd(C.byref(_dv(d, k, ch, c[k])), C.byref(_dv(d, o, ch, c[o])), C.byref(dview), p(d["ddst"]), p(res[k][1]),
                                        c["acc"][j], st)

        def fin():
            for j, k in enumerate("xg"):
                out[f"d_{k}"] = res[k][1][..., _sl(ch, c[k])].cpu().numpy()
                out[f"d_{k}_outside_ok"] = _kept(res[k][0], res[k][1], c[k]["coff"], ch, d[f"prior_{k}"] if c["acc"][j] else None)
    elif group == "bil":
        bf, bt = outbuf(d["prior"].shape, d["prior"] if c["acc"] else None)
        rc = L.lhn_bilinear_bwd(C.byref(_dv(d, "b", ch, c["b"])), C.byref(_dv(d, None, ch, c["dst"], t=d["dst"])), p(d["ddst"]), p(bt), c["acc"],
                                fl(c["slope"]), st)
        fin = lambda: out.update(d_b=bt[..., _sl(ch, c["b"])].cpu().numpy(),                                               # noqa: E731
                                 d_b_outside_ok=_kept(bf, bt, c["b"]["coff"], ch, d["prior"] if c["acc"] else None))
    elif group == "shf":
        dv = c["dst"]
        yf, y = outbuf((n, c["h"], c["w"], dv["cs"] or 2 * ch))
        rc = L.lhn_shuffle2_fwd(C.byref(_dv(d, "a", ch, c["a"])), C.byref(_dv(d, "b", ch, c["b"])), C.byref(_dv(d, None, 2 * ch, dv, t=y)), st)
        fin = lambda: out.update(dst=y[..., _sl(2 * ch, dv)].cpu().numpy(), dst_outside_ok=_kept(yf, y, dv["coff"], 2 * ch))     # noqa: E731
    elif group == "shb":
        dv = c["dst"]
        res = {k: (outbuf(d[f"prior_{k}"].shape, d[f"prior_{k}"] if c["acc"][j] else None) if k in c["which"] else None) for j, k in enumerate("ab")}
        va, vb = (_dv(d, None, ch, c[k], t=d[f"prior_{k}"]) for k in "ab")       # (only the geometry of a and b is read)
        rc = L.lhn_shuffle2_bwd(C.byref(va), C.byref(vb), C.byref(_dv(d, None, 2 * ch, dv, t=d["ddst"])), p(d["ddst"]),
                                p(res["a"][1]) if res["a"] else None, c["acc"][0], p(res["b"][1]) if res["b"] else None, c["acc"][1], st)

        def fin():
            for j, k in enumerate("ab"):
                if res[k]:
                    out[f"d_{k}"] = res[k][1][..., _sl(ch, c[k])].cpu().numpy()
                    out[f"d_{k}_outside_ok"] = _kept(res[k][0], res[k][1], c[k]["coff"], ch, d[f"prior_{k}"] if c["acc"][j] else None)
    elif group == "mp":
        x, yv = c["x"], c["y"]
        yf, y = _alloc((n, yv["h"], yv["w"], yv["cs"] or ch), dev)
        vx, vy = _dv(d, "x", ch, x), _dv(d, None, ch, yv, t=y)
        if not expect_fail:
            _lib.check(L.lhn_maxpool2_fwd(C.byref(vx), C.byref(vy), st), f"maxpool fwd {name}")
        xf, dx = outbuf(d["prior"].shape, d["prior"] if c["acc"] else None)
        sums = _Sums(d["save"], ch, dev) if c.get("bns") else None
        ad = None
        if c.get("same") or c.get("pooled"):
            ad = GradAdds()
            if c.get("same"):
                ad.same, ad.same_cstride, ad.same_coff = d["same"].data_ptr(), c["same"][0], c["same"][1]
            if c.get("pooled"):
                ad.pooled, (ad.OH, ad.OW, ad.pooled_cstride, ad.pooled_coff) = d["pooled"].data_ptr(), c["pooled"]
        rc = L.lhn_maxpool2_bwd3(C.byref(vx), C.byref(vy), p(d["dy"]), p(dx), c["acc"], C.byref(sums.s) if sums else None,
                                 C.byref(ad) if ad is not None else None, st)

        def fin():
            out.update(y=y[..., _sl(ch, yv)].cpu().numpy(), y_outside_ok=_kept(yf, y, yv["coff"], ch), dx=dx[..., _sl(ch, x)].cpu().numpy(),
                       dx_outside_ok=_kept(xf, dx, x["coff"], ch, d["prior"] if c["acc"] else None))
            if sums:
                sums.folded(out)
    elif group == "apf":
        x, OH, OW = c["x"], c["OH"], c["OW"]
        ocs, ocoff = c.get("ocs", ch), c.get("ocoff", 0)
        of, o = outbuf((n, OH, OW, ocs))
        xt, cc = d["x"], c.get("copy_c", 0)
        if c.get("copy"):
            xt = d["x"].clone()
            xt[..., :cc] = PREFILL                   # the pass-through half: nobody has written it yet
        xf, xb = outbuf(xt.shape, xt)
        vx = _dv(d, "x", ch, x, t=xb)
        pf, ps = outbuf((n * OH * OW, 2, ch)) if "stat" in c else (None, None)
        if "stat" in c or c.get("copy"):
            sl = _slices(c, d)
            rc = L.lhn_avgpool_fwd4(C.byref(vx), p(o), OH, OW, p(ps), C.byref(sl), C.byref(_dv(d, "src", cc, c["copy"])) if c.get("copy") else None, st)
        else:
            rc = L.lhn_avgpool_fwd2(C.byref(vx), p(o), OH, OW, ocs, ocoff, st)

        def fin():
            out.update(pooled=o[..., ocoff:ocoff + ch].cpu().numpy(), pooled_outside_ok=_kept(of, o, ocoff, ch))
            out["x_rest_ok"] = np.array(torch.equal(xb[..., cc:], xt[..., cc:]) and bool((xf[xb.numel():] == PREFILL).all()) and
                                        (bool(cc) or torch.equal(xb, xt)))
            if cc:
                out["x_copied"] = xb[..., :cc].cpu().numpy()
            if ps is not None:
                q = ps.view(n, OH, OW, 2, ch)
                out.update(M0=q[:, :, :, 0].cpu().numpy(), M1=q[:, :, :, 1].cpu().numpy(), pstat_tail_ok=np.array(bool((pf[ps.numel():] == PREFILL).all())))
    elif group == "apb":
        x = c["x"]
        xf, dx = outbuf(d["prior"].shape, d["prior"] if c["acc"] else None)
        sums = _Sums(d["save"], ch, dev) if c.get("bns") else None
        rc = L.lhn_avgpool_bwd3(C.byref(_dv(d, "x", ch, x)), p(d["dout"]), c["OH"], c["OW"], c.get("ocs", ch), c.get("ocoff", 0), p(dx), c["acc"],
                                C.byref(sums.s) if sums else None, st)

        def fin():
            out.update(dx=dx[..., _sl(ch, x)].cpu().numpy(), dx_outside_ok=_kept(xf, dx, x["coff"], ch, d["prior"] if c["acc"] else None))
            if sums:
                sums.folded(out)
    elif group == "gate":
        y, parts = c["y"], 3 if c.get("tsum") else 1
        gf, gt = outbuf((parts, n * ch), None if not c["pre"] else torch.zeros(parts, n * ch))
        tsum = C.c_void_p(gt.data_ptr() + 4 * (n * ch + c.get("tsum_off", 0))) if c.get("tsum") else None
        sl = _slices(c, d)
        rc = L.lhn_gate_bwd_reduce3(C.byref(_dv(d, "y", ch, y)), p(d["dz"]), p(gt), tsum, C.byref(sl), c["pre"], st)

        def fin():
            out.update(dgate=gt[0].view(n, ch).cpu().numpy(), dgate_tail_ok=np.array(bool((gf[gt.numel():] == PREFILL).all())))
            if c.get("tsum"):
                t = gt[1:].reshape(n, 2, ch)
                out.update(T0=t[:, 0].cpu().numpy(), T1=t[:, 1].cpu().numpy())
    torch.cuda.synchronize()
    if expect_fail:
        return rc, all(torch.equal(a, b) for a, b in wrote)
    _lib.check(rc, f"{group}:{name}")
    fin()
    return out


# ---------------------------------------------------------------- calls the library must refuse
def _with(group, name, **kw):
    c = dict(GROUPS[group][name], **kw)
    return group, name, c


REFUSE = {    # name: (group, base case, refused variant, text lhn_last_error must hold)
    "bilinear_bwd_silu": _with("bil", "4x5_leaky", slope=SILU) + ("SiLU / ReLU-sigmoid",),
    "bilinear_bwd_relu_sigmoid": _with("bil", "4x5_leaky", slope=RSIG) + ("SiLU / ReLU-sigmoid",),
    "ew_bwd_list_silu_upsampled": _with("ewb", "list_skip", slope=SILU) + ("same-size source",),
    "ew_bwd_list_relu_sigmoid_upsampled": _with("ewb", "list_skip", slope=RSIG) + ("same-size source",),
    "avgpool_bwd_OH_3H": _with("apb", "full_size", OH=15, OW=6) + ("pooled size",),
    "avgpool_bwd_OW_gt_W": _with("apb", "full_size", OH=5, OW=7) + ("pooled size",),
    "avgpool_bwd_OH_0": _with("apb", "full_size", OH=0, OW=6) + ("pooled size",),
    "avgpool_bwd_cstride_mod4": _with("apb", "full_size", ocs=18) + ("multiples of 4",),
    "avgpool_bwd_coff_mod4": _with("apb", "full_size", ocs=20, ocoff=2) + ("multiples of 4",),
    "maxpool_adds_odd": _with("mp", "7x9_c20", same=(24, 4), bns=False) + ("even H, W",),
    "ew_bwd_multi_silu": _with("ewb", "multi2_identity", slope=SILU) + ("lhn_ew_bwd_multi: SiLU",),
    "ew_bwd3_fanout": _with("ewb", "fan2x3", srcs=[S(V(3, 3))]) + ("non-integer upsample",),
    "ew_mul_bwd_fanout": _with("mul", "product", g=V(3, 4, 48, 4, tab=True, gate=True)) + ("non-integer upsample",),
    "gate_tsum_detached": _with("gate", "tsum_two_slices", tsum_off=4) + ("behind dgate",),
    "avgpool_stat_on_slice": _with("apf", "stat", x=V(16, 24, 72, 8, tab=True)) + ("pool a whole buffer",),
    "avgpool_copy_on_slice": _with("apf", "copy", x=V(16, 24, 72, 8, tab=True)) + ("pool a whole buffer",),
}


def refuse_inputs(key):
    """Inputs of a refused variant: those of its own geometry (the variant replaces the case for the length of the call)."""
    group, name, c, _ = REFUSE[key]
    saved = GROUPS[group][name]
    GROUPS[group][name] = c
    try:
        g = inputs(group, name)
        if group == "apb":                 # dout as the call describes it
            g["dout"] = _rand((c["n"], max(c["OH"], 1), c["OW"], c.get("ocs", c["c"])), 99)
    finally:
        GROUPS[group][name] = saved
    return g


# ---------------------------------------------------------------- which kernel, instance and path a case reaches
def instance_of(group, name):
    c = GROUPS[group][name]
    ch = c["c"]
    c4 = ch // 4
    flush = lambda: "atomics flush" if c4 <= 32 and c4 & (c4 - 1) == 0 else "LDS flush"     # noqa: E731
    if group == "ewf":
        bil = bool(c.get("mode", 0) & 2)
        w, pl = c["dst"]["w"], 256 // c4
        path = "bilinear loop" if bil else f"plain loop, {math.ceil(w / (4 * pl))} pass(es)" + (" with a tail" if w % (4 * pl) and w > 4 * pl else "")
        return f"k_ew_fwd<{'true' if bil else 'false'}>", f"{path}; PL = {pl}" + ("; dead threads" if 256 % c4 else "")
    if group == "ewb":
        api = c.get("api", "bwd3")
        bns = [flush() for s in c["srcs"] if s["bns"]]
        kern = "k_ew_bwd_multi" if api == "multi" else "k_ew_bwd_src" + (f" x {sum(not s['skip'] for s in c['srcs'])}" if api == "list" else "")
        return kern, "; ".join(["leaky from dst" if c["slope"] not in (SILU, RSIG, 1.0) else {SILU: "SiLU recompute", RSIG: "ReLU-sigmoid recompute", 1.0: "identity"}[c["slope"]]]
                               + (["dpool"] if c.get("dpool") else []) + bns[:1])
    if group == "mul":
        return "k_ew_mul_bwd x 2", "big operand reads the small one; small operand sums its fan-out"
    if group == "bil":
        return "k_bilinear_bwd", "leaky from dst" if c["slope"] != 1.0 else "identity"
    if group == "shf":
        return "k_shuffle2_fwd", "tables + gates" if c["a"]["tab"] else "plain move"
    if group == "shb":
        return "k_shuffle2_bwd", "d" + c["which"]
    if group == "mp":
        add = bool(c.get("same") or c.get("pooled"))
        return f"k_maxpool2_fwd, k_maxpool2_bwd<{'true' if add else 'false'}>", "; ".join((["addends"] if add else []) + ([flush()] if c.get("bns") else [])) or "plain"
    if group == "apf":
        x = c["x"]
        small = (-(-x["h"] // c["OH"]) + 1) * (-(-x["w"] // c["OW"]) + 1) <= 25 and "stat" not in c and not c.get("copy")
        if small:
            return "k_avgpool_small", "one thread per (bin, 4 channels)"
        red = "shuffle reduction" if c4 <= 64 and c4 & (c4 - 1) == 0 else "LDS reduction"
        return f"k_avgpool_fwd<{'true' if 'stat' in c else 'false'},{'true' if c.get('copy') else 'false'}>", f"workgroup per bin; {red}; PL = {256 // c4}"
    if group == "apb":
        return "k_avgpool_bwd", flush() if c.get("bns") else "plain"
    y = c["y"]
    return "k_gate_bwd_reduce", f"{min(max((y['h'] * y['w'] + 127) // 128, 1), 32)} chunk(s)" + ("; tsum" if c.get("tsum") else "")


def _print_instances():
    print("| group | case | kernel | path |\n|---|---|---|---|")
    for grp, tab in GROUPS.items():
        for nm in tab:
            k, path = instance_of(grp, nm)
            print(f"| {grp} | {nm} | `{k}` | {path} |")


# ---------------------------------------------------------------- input conditions (CPU)
def _sign_ok(t32, t64, what):
    for t in (t32, t64):
        lim = MARGIN * float(t.abs().max())
        assert bool(((t == 0) | (t.abs() >= lim)).all()), f"{what}: a value within {MARGIN} of 0"
    assert bool(((t32 == 0) == (t64 == 0)).all()) and bool(((t32 > 0) == (t64 > 0)).all()), f"{what}: float32 and float64 disagree about a sign"


def check_conditions(group, name, g):
    c = GROUPS[group][name]
    for key in g.get("_kinks", []):
        t = g[key + "_tab"]
        _sign_ok(g[key] * t[0] + t[1], g[key].double() * t[0].double() + t[1].double(), f"{group}:{name} {key}")
    for key in g.get("_signs", []):
        _sign_ok(g[key], g[key].double(), f"{group}:{name} {key}")
    if group == "bil":
        _sign_ok(_bil_pre(c, g, torch.float32), _bil_pre(c, g, torch.float64), f"{group}:{name} pre-activation")
        assert torch.equal(g["dst"][..., _sl(c["c"], c["dst"])] > 0, _bil_pre(c, g, torch.float64) > 0)
    if group == "mp":
        x = c["x"]
        v32, v64 = _val(g, "x", c["c"], x, torch.float32), _val(g, "x", c["c"], x, torch.float64)
        assert torch.equal(v32.double(), v64), f"{group}:{name}: the grid values differ between float32 and float64"
        t = g["x_tab"]
        _sign_ok(g["x"] * t[0] + t[1], g["x"].double() * t[0].double() + t[1].double(), f"{group}:{name} x")
        hp, wp = x["h"] % 2, x["w"] % 2
        win = F.pad(_nchw(v64), (0, wp, 0, hp), value=-float("inf")).unfold(2, 2, 2).unfold(3, 2, 2).reshape(c["n"], c["c"], -1, 4)
        top = win.sort(-1, descending=True).values
        gap = top[..., 0] - top[..., 1]
        assert bool(((gap == 0) | (gap >= MARGIN * float(v64.abs().max()))).all()), f"{group}:{name}: a window's maximum leads by less than {MARGIN}"
        if x["slope"] == 0.0:
            assert bool(((top[..., 0] == 0) & (top[..., 3] == 0)).any()), f"{group}:{name}: no window ties at exactly 0"


def _nearest_rule_ok(i, o):
    """F.interpolate(nearest) in float64 follows the float32 rule min(floor(d * (float)in/out), in - 1)."""
    got = F.interpolate(torch.arange(i, dtype=torch.float64).view(1, 1, 1, i), size=(1, o), mode="nearest").view(-1).long()
    sc = np.float32(i) / np.float32(o)
    rule = np.minimum(np.floor(np.arange(o, dtype=np.float32) * sc).astype(np.int64), i - 1)
    exact = (np.arange(o) * i) // o
    return bool((got.numpy() == rule).all()), bool((rule != exact).any())


def _check_reference():
    import time
    t0 = time.time()
    for i, o in ((6, 74), (14, 46)):
        same, differs = _nearest_rule_ok(i, o)
        assert same and differs, f"nearest {i} -> {o}: torch follows the float32 rule: {same}; it differs from the integer rule: {differs}"
    for grp, tab in GROUPS.items():
        worst = 0.0
        for nm in tab:
            g = inputs(grp, nm)
            check_conditions(grp, nm, g)
            r64, r32 = reference(grp, nm, g), reference(grp, nm, g, torch.float32)
            assert r64, f"{grp}:{nm}: no outputs"
            for k in r64:
                assert np.isfinite(r64[k]).all() and np.abs(r64[k]).max() > 0, f"{grp}:{nm} {k}: reference not finite or all zeros"
                if k in exact_keys(grp, nm):
                    continue
                worst = max(worst, rel_err(r32[k], r64[k]))
            instance_of(grp, nm)
        print(f"{grp:5s} {len(tab):3d} cases, worst float32 error {worst:.2e}")
    for full in DET:
        grp, nm = full.split(":")
        assert rows(grp, nm) > 16, f"{full}: {rows(grp, nm)} rows do not make a 16-workgroup grid iterate"
    for key in REFUSE:
        refuse_inputs(key)
    print(f"{sum(len(t) for t in GROUPS.values())} cases, {len(REFUSE)} refusals, input conditions hold, {time.time() - t0:.1f} s")


if __name__ == "__main__":
    if sys.argv[1] == "--check-reference":
        _check_reference()
        sys.exit(0)
    if sys.argv[1] == "--instances":
        _print_instances()
        sys.exit(0)
    dst, reps, names = sys.argv[1], int(sys.argv[2]), sys.argv[3:]
    dev = torch.device("cuda:0")
    res = {}
    for full in names:
        grp, nm = full.split(":")
        g = inputs(grp, nm)
        for r in range(reps):
            for k, v in run(grp, nm, dev, g).items():
                res[f"{full}/{r}/{k}"] = v
    np.savez(dst, **res)
