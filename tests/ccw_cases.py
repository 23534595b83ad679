"""Cases of the four grouped ConditionalChannelWeighting entry points (lhn_ccw_pool_fwd, lhn_ccw_gate_fwd, lhn_ccw_dw_fwd,
lhn_ccw_shuffle_fwd: one launch each over all 2..4 branches of a Lite-HRNet block) run through the C ABI, the launch chains they
replace on the same inputs, and float64 torch references (adaptive_avg_pool2d, F.conv2d(groups=C), F.interpolate(nearest), the
reference's channel_shuffle restated).  Imported by tests/test_ccw_gpu.py; as a script,
    python tests/ccw_cases.py --check-reference        (CPU only: every case's inputs and references)

Every entry point is judged on its own: its inputs are given float32 tensors (the pooled concatenation and the gate map are the
float64 references rounded once; the shuffle reads the y and the tile sums the fused depthwise call left), the chain it replaces
reads the same tensors, and the float64 reference starts from them.

Inputs.  The tables in front of both sigmoid(relu(.)) pairs and the biases of SpatialWeighting's MLP are +-1.5 (alternating) under
pre-activations of a few tenths, so both ReLU branches are taken and no pre-activation sits within MARGIN of the kink: a reference
whose float32 form flips a branch would widen the bar and hide a failure."""
import ctypes as C
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from litehandnet_amd import _lib  # noqa: E402
from litehandnet_amd._lib import CcwSe, View  # noqa: E402

FLOOR = 1e-4                     # the forward floor of test_msrb_round_gpu / test_model_gpu._check_block: of the float64 peak
PREFILL = 7.0
MARGIN = 1e-3                    # no pre-activation of a sigmoid(relu(.)) within this of zero (float64)
RELU_SIGMOID = 3.0               # LHN_SLOPE_RELU_SIGMOID
EW_MUL = 1


class PwOpts(C.Structure):       # lhn_pw_opts (include/lhn.h)
    _fields_ = [("w_cols", C.c_int32), ("w_rows", C.c_int32), ("nchw_batch_stride", C.c_int64), ("n_extra", C.c_int32),
                ("extra", C.c_void_p), ("coef", C.c_float * 3), ("sum_out", C.c_void_p)]


def _case(n, maps, chans, wide=False, xtab=None, xgate=False, const=False, spread=False):
    """maps: (H, W) per branch, largest first; chans: C_b per branch; wide: every view is a channel slice of a wider buffer filled
    with PREFILL; xtab: None | "near" | "neg" (negative scales too) | a shift ("shift far"), slope 0.1; xgate: the inputs carry a
    per-(n, c) gate; const: the exact-arithmetic inputs (see inputs); spread: sample n's inputs are 1 + n times as large and shifted by n, so that
    both gates differ visibly from sample to sample."""
    return dict(n=n, maps=list(maps), chans=list(chans), wide=wide, xtab=xtab, xgate=xgate, const=const, spread=spread, mid=int(sum(chans) / 8))


SQ = lambda *s: [(v, v) for v in s]
CASES = {
    "b2_16_8": _case(2, SQ(16, 8), (20, 40)),
    "b3_16_8_4": _case(3, SQ(16, 8, 4), (20, 40, 80)),
    "b4_stage4_at_64": _case(2, SQ(16, 8, 4, 2), (20, 40, 80, 160)),       # Ct = 300, mid = 37: stage 4 at a 64 x 64 image
    "last_1x1": _case(2, SQ(4, 2, 1), (20, 40, 80)),
    "all_1x1": _case(3, SQ(1, 1), (20, 40)),
    "nonsquare_12x20": _case(2, [(12, 20), (6, 10)], (20, 40)),
    "ratio_1": _case(3, SQ(8, 8, 8), (20, 40, 80)),
    "ratio_3": _case(2, SQ(12, 4), (24, 36)),                              # 9-pixel windows: not a multiple of the lanes that share them
    "ratio_8": _case(1, SQ(32, 4), (20, 40)),                              # 64-pixel windows: four pixels per sharing lane
    "slices_of_wider_buffers": _case(2, SQ(16, 8, 4), (20, 40, 80), wide=True, xtab="near"),
    "negative_scales": _case(2, SQ(16, 8), (20, 40), xtab="neg"),
    "shift_far": _case(2, SQ(16, 8, 4), (20, 40, 80), xtab=5.0),
    "shift_far_negative_1x1": _case(2, SQ(4, 2, 1), (20, 40, 80), xtab=-4.0, wide=True),
    "gated_input": _case(3, SQ(16, 8), (20, 40), xtab="near", xgate=True),
    "per_sample_gates": _case(3, SQ(16, 8, 4), (20, 40, 80), spread=True),
    "const_b3": _case(3, SQ(16, 8, 4), (20, 40, 80), const=True),
    "const_ratio_3": _case(2, [(12, 9), (4, 3)], (24, 36), const=True),
    "const_b4_wide": _case(2, SQ(16, 8, 4, 2), (20, 40, 80, 160), const=True, wide=True),
}


def _rand(shape, seed, scale=1.0):
    return torch.from_numpy((np.random.Generator(np.random.PCG64(seed)).standard_normal(shape) * scale).astype(np.float32))


def _pm(nc, mag=1.5):
    return torch.tensor([mag if j % 2 == 0 else -mag for j in range(nc)], dtype=torch.float32)


def layout(c, b):
    """(x cstride, x1 coff, x2 coff, y cstride, y coff, out cstride, out coff) of branch b."""
    cb, pad = c["chans"][b], 8 if c["wide"] else 0
    o = 4 if c["wide"] else 0
    return 2 * cb + pad, o, o + cb, cb + pad, o, 2 * cb + pad, o


def inputs(name, seed=23):
    """Everything the four calls read, as CPU float32 tensors.  const: x = a small integer per (sample, pooled cell), so window sums,
    their means and the nearest upsample are exact in fp32; the gate map is a power of two per (sample, pooled cell) and every
    depthwise tap is 1, so y is an exact sum of at most nine such numbers: one pixel in the wrong window, one wrong gate cell or a
    mixed-up sample is a bit difference."""
    c = CASES[name]
    n, B, mid, Ct = c["n"], len(c["maps"]), c["mid"], sum(c["chans"])
    hm, wm = c["maps"][-1]
    cp = (mid + 3) // 4 * 4
    g = {}
    cell = (torch.arange(n)[:, None, None] * 3 + torch.arange(hm)[None, :, None] * wm + torch.arange(wm)[None, None, :])
    for b, ((h, w), cb) in enumerate(zip(c["maps"], c["chans"])):
        xcs, _, _, ycs, _, _, _ = layout(c, b)
        if c["const"]:
            up = (1 + cell % 7).float().repeat_interleave(h // hm, 1).repeat_interleave(w // wm, 2)
            g[f"x{b}"] = up[..., None].expand(n, h, w, xcs).contiguous()
            g[f"wdw{b}"] = torch.ones(cb, 1, 3, 3)
        else:
            g[f"x{b}"] = _rand((n, h, w, xcs), seed + 10 * b)
            if c["spread"]:
                g[f"x{b}"] = g[f"x{b}"] * (1.0 + torch.arange(n))[:, None, None, None] + torch.arange(n)[:, None, None, None]
            g[f"wdw{b}"] = _rand((cb, 1, 3, 3), seed + 10 * b + 4, 0.4)
        if c["xtab"] is not None:
            sc = 1 + 0.3 * _rand((xcs,), seed + 10 * b + 1)
            if c["xtab"] == "neg":
                sc = sc * _pm(xcs, 1.0)
            shift = float(c["xtab"]) if not isinstance(c["xtab"], str) else 0.0
            g[f"xtab{b}"] = torch.stack([sc, 0.2 * _rand((xcs,), seed + 10 * b + 2) + shift, torch.full((xcs,), 0.1)]).contiguous()
        if c["xgate"]:
            g[f"xgate{b}"] = torch.sigmoid(_rand((n, xcs), seed + 10 * b + 3))
        g[f"ytab{b}"] = torch.stack([1 + 0.3 * _rand((ycs,), seed + 10 * b + 5), 0.2 * _rand((ycs,), seed + 10 * b + 6) + 0.3, torch.ones(ycs)]).contiguous()
        J = cb // 4
        g[f"se{b}"] = (_rand((J, cb), seed + 10 * b + 7, 0.5 / cb ** 0.5), _pm(J), _rand((cb, J), seed + 10 * b + 8, 0.5 / J ** 0.5), _pm(cb))
    g["w1"], g["w2"] = _rand((mid, Ct), seed + 60, 1.0 / Ct ** 0.5), _rand((Ct, mid), seed + 61, 1.0 / mid ** 0.5)
    t1 = torch.stack([torch.ones(cp), torch.zeros(cp), torch.ones(cp)])
    t1[0, :mid], t1[1, :mid] = 0.3 * (1 + 0.3 * _rand((mid,), seed + 62)), _pm(mid)
    g["t1"] = t1.contiguous()
    g["t2"] = torch.stack([0.3 * (1 + 0.3 * _rand((Ct,), seed + 63)), _pm(Ct), torch.ones(Ct)]).contiguous()
    return g


def value(x, tab, gate):
    x = x.double()
    if tab is not None:
        u = x * tab.double()[0] + tab.double()[1]
        x = torch.where(u > 0, u, u * tab.double()[2])
    if gate is not None:
        x = x * gate.double()[:, None, None, :]
    return x


def relu_sigmoid(v):
    return torch.sigmoid(torch.relu(v))


def channel_shuffle(x, groups):
    """lite_hrnet.py:29-52 restated (NCHW)."""
    n, ch, h, w = x.shape
    return x.view(n, groups, ch // groups, h, w).transpose(1, 2).contiguous().view(n, ch, h, w)


def shuffle_reference(name, g, b, y):
    """float64 (out [N,H,W,2C], pre-activations) of branch b from the raw depthwise output y [N,H,W,C] (float32, as stored)."""
    c = CASES[name]
    cb = c["chans"][b]
    xcs, o1, _, ycs, oy, _, _ = layout(c, b)
    v1 = value(g[f"x{b}"], g.get(f"xtab{b}"), g.get(f"xgate{b}"))[..., o1:o1 + cb]
    t = g[f"ytab{b}"].double()[:, oy:oy + cb]
    vy = y.double() * t[0] + t[1]                        # (slope 1: a BatchNorm without an activation)
    w1, b1, w2, b2 = (p.double() for p in g[f"se{b}"])
    p1 = vy.mean((1, 2)) @ w1.T + b1
    p2 = relu_sigmoid(p1) @ w2.T + b2
    gated = vy * relu_sigmoid(p2)[:, None, None, :]
    out = channel_shuffle(torch.cat([v1, gated], -1).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).contiguous()
    return out, (p1, p2)


def reference(name, g):
    """float64 references of the pool, the gate and the depthwise call, the float32 tensors the latter two read, and every
    pre-activation in front of a sigmoid(relu(.))."""
    c = CASES[name]
    n, B, mid, Ct = c["n"], len(c["maps"]), c["mid"], sum(c["chans"])
    hm, wm = c["maps"][-1]
    v2 = []
    for b, cb in enumerate(c["chans"]):
        _, _, o2, _, _, _, _ = layout(c, b)
        v2.append(value(g[f"x{b}"], g.get(f"xtab{b}"), g.get(f"xgate{b}"))[..., o2:o2 + cb].permute(0, 3, 1, 2))
    pooled = torch.cat([F.adaptive_avg_pool2d(v, (hm, wm)) for v in v2], 1).permute(0, 2, 3, 1).contiguous()
    r = dict(pooled=pooled, pooled_in=pooled.float())
    t1, t2 = g["t1"].double(), g["t2"].double()
    p1 = (r["pooled_in"].double() @ g["w1"].double().T) * t1[0, :mid] + t1[1, :mid]
    p2 = (relu_sigmoid(p1) @ g["w2"].double().T) * t2[0] + t2[1]
    r["g"] = relu_sigmoid(p2)
    if c["const"]:
        cell = (torch.arange(n)[:, None, None] * 5 + torch.arange(hm)[None, :, None] * wm + torch.arange(wm)[None, None, :])
        r["g_in"] = (2.0 ** -(cell % 4).float())[..., None].expand(n, hm, wm, Ct).contiguous()
    else:
        r["g_in"] = r["g"].float()
    pre, off, ys = [p1, p2], 0, []
    for b, ((h, w), cb) in enumerate(zip(c["maps"], c["chans"])):
        up = F.interpolate(r["g_in"].double()[..., off:off + cb].permute(0, 3, 1, 2), size=(h, w), mode="nearest")
        off += cb
        y = F.conv2d(v2[b] * up, g[f"wdw{b}"].double(), padding=1, groups=cb).permute(0, 2, 3, 1).contiguous()
        ys.append(y)
        pre += list(shuffle_reference(name, g, b, y.float())[1])
    r["y"], r["pre"] = ys, pre
    return r


_REFS = {}


def ref(name):
    """(inputs, references) of a case: computed once, shared by the tests, never modified."""
    if name not in _REFS:
        g = inputs(name)
        _REFS[name] = (g, reference(name, g))
    return _REFS[name]


def view(t, coff, c, table=None, gate=None):
    v = View()
    v.data, v.table, v.gate, v.pend = t.data_ptr(), (table.data_ptr() if table is not None else None), \
        (gate.data_ptr() if gate is not None else None), None
    v.N, v.H, v.W, v.cstride, v.coff, v.C = t.shape[0], t.shape[1], t.shape[2], t.shape[3], coff, c
    return v


class Device:
    """The inputs of a case on the GPU and the views the calls take."""

    def __init__(self, name, g, r, dev):
        c = self.c = CASES[name]
        self.dev, self.n, self.B, self.mid, self.Ct = dev, c["n"], len(c["maps"]), c["mid"], sum(c["chans"])
        self.hm, self.wm = c["maps"][-1]
        self.d = {k: (tuple(t.to(dev) for t in v) if isinstance(v, tuple) else v.to(dev)) for k, v in g.items()}
        self.pooled_in, self.g_in = r["pooled_in"].to(dev), r["g_in"].to(dev)
        self.lay = [layout(c, b) for b in range(self.B)]
        self.offs = [sum(c["chans"][:b]) for b in range(self.B)]

    def x(self, b, which):
        cb, d = self.c["chans"][b], self.d
        return view(d[f"x{b}"], self.lay[b][1 if which == 1 else 2], cb, d.get(f"xtab{b}"), d.get(f"xgate{b}"))

    def xs(self, which):
        return (View * self.B)(*[self.x(b, which) for b in range(self.B)])

    def fresh(self, what):
        """PREFILL-filled output buffers, one per branch: "y" or "out"."""
        return [torch.full((self.n, h, w, self.lay[b][3 if what == "y" else 5]), PREFILL, device=self.dev)
                for b, (h, w) in enumerate(self.c["maps"])]

    def yv(self, ys, b, gate=None):
        return view(ys[b], self.lay[b][4], self.c["chans"][b], self.d[f"ytab{b}"], gate)

    def ov(self, outs, b):
        return view(outs[b], self.lay[b][6], 2 * self.c["chans"][b])

    def scratch_floats(self):
        arr = lambda vals: (C.c_int * self.B)(*vals)
        nbytes = _lib.lib().lhn_ccw_scratch_bytes(self.n, self.B, arr(m[0] for m in self.c["maps"]), arr(m[1] for m in self.c["maps"]),
                                                  arr(self.c["chans"]))
        assert nbytes > 0 and nbytes % 4 == 0
        return nbytes // 4


def run_fused(D):
    """The four grouped calls.  Returns pooled, g, the y buffers, the scratch (floats, PREFILL behind its end) and the out buffers."""
    L, d, B = _lib.lib(), D.d, D.B
    pooled = torch.full((D.n, D.hm, D.wm, D.Ct), PREFILL, device=D.dev)
    _lib.check(L.lhn_ccw_pool_fwd(D.xs(2), B, _lib.ptr(pooled), _lib.stream()), "lhn_ccw_pool_fwd")
    gate = torch.full((D.n, D.hm, D.wm, D.Ct), PREFILL, device=D.dev)
    _lib.check(L.lhn_ccw_gate_fwd(_lib.ptr(D.pooled_in), D.n * D.hm * D.wm, D.Ct, D.mid, _lib.ptr(d["w1"]), _lib.ptr(d["t1"]), d["t1"].shape[1],
                                  _lib.ptr(d["w2"]), _lib.ptr(d["t2"]), D.Ct, _lib.ptr(gate), _lib.stream()), "lhn_ccw_gate_fwd")
    ys, nf = D.fresh("y"), D.scratch_floats()
    scratch = torch.full((nf + 64,), PREFILL, device=D.dev)
    ws = (C.c_void_p * B)(*[d[f"wdw{b}"].data_ptr() for b in range(B)])
    yv = (View * B)(*[D.yv(ys, b) for b in range(B)])
    _lib.check(L.lhn_ccw_dw_fwd(D.xs(2), B, _lib.ptr(D.g_in), ws, yv, _lib.ptr(scratch), _lib.stream()), "lhn_ccw_dw_fwd")
    outs = D.fresh("out")
    _lib.check(shuffle_call(D, ys, scratch, outs), "lhn_ccw_shuffle_fwd")
    torch.cuda.synchronize()
    return dict(pooled=pooled.cpu(), g=gate.cpu(), y=[t.cpu() for t in ys], scratch=scratch.cpu(), out=[t.cpu() for t in outs], y_dev=ys)


def shuffle_call(D, ys, scratch, outs, B=None, x1=None, se=None):
    B = D.B if B is None else B
    ses = se if se is not None else (CcwSe * D.B)()
    if se is None:
        for b in range(D.B):
            w1, b1, w2, b2 = D.d[f"se{b}"]
            ses[b].w1, ses[b].b1, ses[b].w2, ses[b].b2, ses[b].J = w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), w1.shape[0]
    yv = (View * D.B)(*[D.yv(ys, b) for b in range(D.B)])
    ov = (View * D.B)(*[D.ov(outs, b) for b in range(D.B)])
    return _lib.lib().lhn_ccw_shuffle_fwd(x1 if x1 is not None else D.xs(1), yv, B, ses, None if scratch is None else _lib.ptr(scratch), ov, _lib.stream())


def run_chain(D, ys_in):
    """The launches the four calls replace, on the same inputs: B average pools into the concatenation; 1x1, combine, 1x1, combine;
    B products and B depthwise convolutions; B x (global pool, SE MLP mode 1, shuffle) reading ys_in (the fused call's y)."""
    L, d, B, c, st = _lib.lib(), D.d, D.B, D.c, _lib.stream()
    one, rs = C.c_float(1.0), C.c_float(RELU_SIGMOID)
    pooled = torch.full((D.n, D.hm, D.wm, D.Ct), PREFILL, device=D.dev)
    for b in range(B):
        xv = D.x(b, 2)
        _lib.check(L.lhn_avgpool_fwd2(C.byref(xv), _lib.ptr(pooled), D.hm, D.wm, D.Ct, D.offs[b], st), "lhn_avgpool_fwd2")
    cp, pad = d["t1"].shape[1], D.mid % 4 != 0
    a_raw, a = (torch.zeros((D.n, D.hm, D.wm, cp), device=D.dev) for _ in range(2))
    g_raw, gate = (torch.zeros((D.n, D.hm, D.wm, D.Ct), device=D.dev) for _ in range(2))
    o1, o2 = PwOpts(w_rows=D.mid if pad else 0), PwOpts(w_cols=D.mid if pad else 0)
    pin, av, arv, grv, gv = view(D.pooled_in, 0, D.Ct), view(a, 0, cp), view(a_raw, 0, cp), view(g_raw, 0, D.Ct), view(gate, 0, D.Ct)
    _lib.check(L.lhn_conv_pw_fwd2(C.byref(pin), _lib.ptr(d["w1"]), None, C.byref(arv), None, 1, None, None, C.byref(o1), st), "lhn_conv_pw_fwd2")
    _lib.check(L.lhn_ew_fwd3((View * 1)(view(a_raw, 0, cp, d["t1"])), 1, None, C.byref(av), rs, 0, st), "lhn_ew_fwd3")
    _lib.check(L.lhn_conv_pw_fwd2(C.byref(av), _lib.ptr(d["w2"]), None, C.byref(grv), None, 1, None, None, C.byref(o2), st), "lhn_conv_pw_fwd2")
    _lib.check(L.lhn_ew_fwd3((View * 1)(view(g_raw, 0, D.Ct, d["t2"])), 1, None, C.byref(gv), rs, 0, st), "lhn_ew_fwd3")
    ys, outs = D.fresh("y"), D.fresh("out")
    for b, ((h, w), cb) in enumerate(zip(c["maps"], c["chans"])):
        prod = torch.zeros((D.n, h, w, cb), device=D.dev)
        pv, yv = view(prod, 0, cb), D.yv(ys, b)
        _lib.check(L.lhn_ew_fwd3((View * 2)(D.x(b, 2), view(D.g_in, D.offs[b], cb)), 2, None, C.byref(pv), one, EW_MUL, st), "lhn_ew_fwd3")
        _lib.check(L.lhn_conv_dw_fwd3(C.byref(pv), _lib.ptr(d[f"wdw{b}"]), C.byref(yv), None, 3, 1, 1, 1, None, None, None, None, st), "lhn_conv_dw_fwd3")
        w1, b1, w2, b2 = d[f"se{b}"]
        J, ycs, oy = w1.shape[0], D.lay[b][3], D.lay[b][4]
        p1, sg, save = torch.zeros((D.n, 1, 1, cb), device=D.dev), torch.zeros((D.n, ycs), device=D.dev), torch.zeros(D.n * (J + cb), device=D.dev)
        yin, x1v, ov = D.yv(ys_in, b), D.x(b, 1), D.ov(outs, b)
        _lib.check(L.lhn_avgpool_fwd(C.byref(yin), _lib.ptr(p1), 1, 1, st), "lhn_avgpool_fwd")
        _lib.check(L.lhn_se_mlp_fwd2(_lib.ptr(p1), _lib.ptr(w1), _lib.ptr(b1), _lib.ptr(w2), _lib.ptr(b2), _lib.ptr(sg), ycs, oy, _lib.ptr(save),
                                     D.n, cb, J, 1, st), "lhn_se_mlp_fwd2")
        ygv = D.yv(ys_in, b, sg)
        _lib.check(L.lhn_shuffle2_fwd(C.byref(x1v), C.byref(ygv), C.byref(ov), st), "lhn_shuffle2_fwd")
    torch.cuda.synchronize()
    return dict(pooled=pooled.cpu(), g=gate.cpu(), y=[t.cpu() for t in ys], out=[t.cpu() for t in outs])


def check_reference():
    """CPU only: shapes, finiteness, non-degenerate references, both ReLU branches taken and no pre-activation near the kink."""
    for name, c in CASES.items():
        g, r = ref(name)
        n, Ct = c["n"], sum(c["chans"])
        hm, wm = c["maps"][-1]
        assert r["pooled"].shape == (n, hm, wm, Ct) == r["g"].shape and c["mid"] == int(Ct / 8) <= 40 and Ct <= 320, name
        for (h, w), cb, y in zip(c["maps"], c["chans"], r["y"]):
            assert h % hm == 0 and w % wm == 0 and cb % 4 == 0 and cb <= 160 and y.shape == (n, h, w, cb), name
            assert bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0.05, name
        for p in r["pre"]:
            assert float(p.abs().min()) > MARGIN, (name, float(p.abs().min()))
            assert bool((p > 0).any()) and bool((p < 0).any()), name
        if c["const"]:
            assert torch.equal(r["pooled"], r["pooled"].round()) and torch.equal(r["pooled"].float().double(), r["pooled"]), name
            assert all(torch.equal(y.float().double(), y) for y in r["y"]), name
        print(f"{name}: ok, closest pre-activation {min(float(p.abs().min()) for p in r['pre']):.3e}")


if __name__ == "__main__":
    assert sys.argv[1:] == ["--check-reference"], __doc__
    check_reference()
