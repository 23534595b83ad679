"""Case table, inputs and float64 reference of lhn_stem_tail_fwd (tests/test_stem_tail_gpu.py runs them on the GPU,
tests/test_infer_fuse_stem_cpu.py checks on the CPU that no guarding case is degenerate).  Importable without a GPU and without liblhn.so.

A case is one call, m = 32, C = 128, on an H x W map at t level:
    t = K ? actT(dwKxK(value(x)) + bT) : value(x)      u = actU(w1 . t + b1)      v = actV(conv3x3 stride 2 (u) + b2)
    p = maxpool2x2 ceil (t)                            y = w3 . cat(v, p) + b3     at ceil(H/2) x ceil(W/2)
`reference(name, g, wrong=...)` is the arithmetic of a kernel that gets one of the four traps wrong:
    "u_pad"            u padded with actU(shift_U) instead of zeros      (visible in the shift_far cases, first row / column of y)
    "x_pad"            x padded with act(shift_x) * gate instead of zeros (xshift_far cases, K > 0)
    "pool_zero"        a 0 standing in for the missing pixels of a clipped pooling window (pool_negative_17x17: t < 0)
    "table_after_max"  the table of t applied after the max instead of before (mixed_sign cases: negative scales)"""
import numpy as np
import torch
import torch.nn.functional as F

M = 32
C_OUT = 128
KS = (0, 3, 7)
FLOOR = 1e-4       # of the output's peak: the forward floor of test_dw3_pw_gpu / test_bottleneck_gpu
PREFILL = 7.0
WRONG = ("u_pad", "x_pad", "pool_zero", "table_after_max")


def _case(k, n, h, w, x=None, y=None, tabs=(True, True, True), biases=(True, True, True, True), slopes=(0.01, 0.01, 0.01),
          shift_far=False, xshift_far=False, xtab=False, xgate=False, mixed=False, pool_negative=False):
    """x, y: (cstride, coff) of the views (default: whole 32- / 128-channel buffers); tabs: tT, tU, tV given; biases: bT, b1, b2, b3
    given; slopes: the slopes in tT, tU, tV; shift_far: tU's shifts are +-(4..5); xshift_far: the shifts of x's own table are;
    mixed: every table's scales alternate in sign; pool_negative: t is strictly negative."""
    return dict(k=k, n=n, h=h, w=w, x=x or (M, 0), y=y or (C_OUT, 0), tabs=tuple(tabs), biases=tuple(biases), slopes=tuple(slopes),
                shift_far=shift_far, xshift_far=xshift_far, xtab=xtab or xshift_far, xgate=xgate, mixed=mixed, pool_negative=pool_negative)


MAPS = ((5, 1, 1), (5, 1, 5), (5, 2, 3), (4, 3, 3), (3, 7, 7), (3, 8, 8), (2, 16, 16), (2, 17, 17), (2, 18, 18), (2, 28, 28), (2, 9, 70),
        (2, 24, 40), (2, 37, 19))
CASES = {}
for _k in KS:
    for _n, _h, _w in MAPS:
        CASES[f"map_{_h}x{_w}_k{_k}"] = _case(_k, _n, _h, _w)
    CASES.update({
        f"x_slice_256_table_gate_k{_k}": _case(_k, 2, 18, 18, x=(256, 64), xtab=True, xgate=True),
        f"y_slice_256_k{_k}": _case(_k, 2, 16, 16, y=(256, 64)),
        f"tT_null_k{_k}": _case(_k, 2, 8, 8, tabs=(False, True, True)),
        f"tU_null_k{_k}": _case(_k, 2, 8, 8, tabs=(True, False, True)),
        f"tV_null_k{_k}": _case(_k, 2, 8, 8, tabs=(True, True, False)),
        f"bT_null_k{_k}": _case(_k, 2, 8, 8, biases=(False, True, True, True)),
        f"b1_null_k{_k}": _case(_k, 2, 8, 8, biases=(True, False, True, True)),
        f"b2_null_k{_k}": _case(_k, 2, 8, 8, biases=(True, True, False, True)),
        f"b3_null_k{_k}": _case(_k, 2, 8, 8, biases=(True, True, True, False)),
        f"all_null_k{_k}": _case(_k, 2, 7, 7, tabs=(False, False, False), biases=(False, False, False, False)),
        f"slopes_0_k{_k}": _case(_k, 2, 17, 17, slopes=(0.0, 0.0, 0.0)),
        f"slopes_1_k{_k}": _case(_k, 2, 17, 17, slopes=(1.0, 1.0, 1.0)),
        f"mixed_sign_k{_k}": _case(_k, 2, 17, 17, mixed=True, xtab=True, x=(64, 32)),
        f"shift_far_8x8_k{_k}": _case(_k, 2, 8, 8, shift_far=True),
        f"shift_far_17x17_k{_k}": _case(_k, 2, 17, 17, shift_far=True, x=(256, 64), xtab=True, xgate=True),
        f"shift_far_12x70_k{_k}": _case(_k, 2, 12, 70, shift_far=True),
        f"pool_negative_17x17_k{_k}": _case(_k, 2, 17, 17, pool_negative=True),
        # Multi-round: the launcher's work item is one 4 x 8 tile of y of one image = one workgroup (4 waves) of 52,768 B (K = 0), 53,280 B
        # (K = 3) or 77,984 B (K = 7) of LDS, so at most three workgroups are resident on a CU and one resident round is at most
        # 3 x 256 = 768 workgroups.  780 images of 4 x 4 (y: 2 x 2, one tile each) are 780 workgroups: more than one round for every K.
        f"multi_round_n780_4_k{_k}": _case(_k, 780, 4, 4),
        # the largest: t of the 224 x 224 configuration
        f"map_112x112_k{_k}": _case(_k, 2, 112, 112),
    })
    if _k:
        CASES[f"xshift_far_17x17_k{_k}"] = _case(_k, 2, 17, 17, xshift_far=True, xgate=True)
        CASES[f"xshift_far_8x8_k{_k}"] = _case(_k, 3, 8, 8, xshift_far=True, x=(64, 32))


def _rand(shape, seed, scale=1.0):
    return torch.from_numpy((np.random.Generator(np.random.PCG64(seed)).standard_normal(shape) * scale).astype(np.float32))


def _alt(k):
    return torch.tensor([1.0 if j % 2 == 0 else -1.0 for j in range(k)])


def _far(ch, seed):
    u = np.random.Generator(np.random.PCG64(seed)).uniform(4.0, 5.0, ch).astype(np.float32)
    return torch.from_numpy(u) * _alt(ch)


def inputs(name, seed=29):
    """CPU float32 tensors of a case: x [N,H,W,xcs], w1, w2, w3 and, where the case has them, w_dw, bT, b1, b2, b3, tT, tU, tV, xtab, xgate."""
    c = CASES[name]
    k, xcs = c["k"], c["x"][0]
    g = {"x": _rand((c["n"], c["h"], c["w"], xcs), seed),
         "w1": _rand((M, M), seed + 1, M ** -0.5),
         "w2": _rand((M, M, 3, 3), seed + 2, (9 * M) ** -0.5 * 1.5),
         "w3": _rand((C_OUT, 2 * M), seed + 3, (2 * M) ** -0.5 * 1.5)}
    if k:
        g["w_dw"] = _rand((M, 1, k, k), seed + 4, 1.5 / k)
    for j, key in enumerate(("bT", "b1", "b2", "b3")):
        if c["biases"][j] and (k or key != "bT"):
            g[key] = 0.3 * _rand((C_OUT if key == "b3" else M,), seed + 5 + j)
    for j, key in enumerate(("tT", "tU", "tV")):
        if c["tabs"][j] and (k or key != "tT"):
            scale = 1 + 0.3 * _rand((M,), seed + 10 + 2 * j)
            shift = 0.2 * _rand((M,), seed + 11 + 2 * j)
            if key == "tU" and c["shift_far"]:
                shift = _far(M, seed + 20)
            if c["mixed"]:
                scale = scale.abs() * _alt(M)
            if key == "tT" and c["pool_negative"]:
                shift = shift - 40.0
            g[key] = torch.stack([scale, shift, torch.full((M,), float(c["slopes"][j]))]).contiguous()
    if c["pool_negative"]:
        if k:
            g["tT"][2] = 1.0        # t = scale * (dw + bT) + shift, far below zero
        else:
            g["x"] = -g["x"].abs() - 0.1
    if c["xtab"]:
        scale = 1 + 0.3 * _rand((xcs,), seed + 30)
        if c["mixed"]:
            scale = scale.abs() * _alt(xcs)
        shift = _far(xcs, seed + 31) if c["xshift_far"] else 0.2 * _rand((xcs,), seed + 31)
        g["xtab"] = torch.stack([scale, shift, torch.full((xcs,), 0.1)]).contiguous()
    if c["xgate"]:
        g["xgate"] = torch.sigmoid(_rand((c["n"], xcs), seed + 32))
    return g


def _act(u, tab):
    """(activated, pre-activation) of an NCHW double tensor under a [3][ch] table (None: identity)."""
    if tab is None:
        return u, u
    t = tab.double()
    p = u * t[0][None, :, None, None] + t[1][None, :, None, None]
    return torch.where(p > 0, p, p * t[2][None, :, None, None]), p


def _bias(g, key):
    return g[key].double() if key in g else None


def reference(name, g, wrong=None, parts=False):
    """float64 NHWC result (F.conv2d / F.max_pool2d on NCHW doubles).  parts=True: also the pre-activation tensors of t (K > 0), u, v
    and t itself."""
    assert wrong is None or wrong in WRONG
    c = CASES[name]
    k, (xcs, xoff), h, w = c["k"], c["x"], c["h"], c["w"]
    raw = g["x"].double().permute(0, 3, 1, 2)                                     # NCHW, all xcs channels
    xt = g["xtab"][:, xoff:xoff + M] if "xtab" in g else None
    gate = g["xgate"].double()[:, xoff:xoff + M, None, None] if "xgate" in g else 1.0
    raw = raw[:, xoff:xoff + M]
    xv = _act(raw, xt)[0] * gate
    pt = None
    if k:
        wd = g["w_dw"].double()
        if wrong == "x_pad":
            pad = _act(torch.zeros(1, M, 1, 1, dtype=torch.float64), xt)[0] * gate      # what a transformed zero-padded raw tile holds
            d = F.conv2d(F.pad(xv - pad, (k // 2,) * 4) + pad, wd, groups=M)
        else:
            d = F.conv2d(xv, wd, padding=k // 2, groups=M)
        if "bT" in g:
            d = d + g["bT"].double()[None, :, None, None]
        t, pt = _act(d, g.get("tT"))
        pool_src, pool_tab = d, g.get("tT")
    else:
        t = xv
        pool_src, pool_tab = raw, xt
    u, pu = _act(F.conv2d(t, g["w1"].double()[:, :, None, None], _bias(g, "b1")), g.get("tU"))
    if wrong == "u_pad":
        pad = _act(torch.zeros(1, M, 1, 1, dtype=torch.float64), g.get("tU"))[0]
        s = F.conv2d(F.pad(u - pad, (1, 1, 1, 1)) + pad, g["w2"].double(), _bias(g, "b2"), stride=2)
    else:
        s = F.conv2d(u, g["w2"].double(), _bias(g, "b2"), stride=2, padding=1)
    v, pv = _act(s, g.get("tV"))
    if wrong == "pool_zero":
        p = F.max_pool2d(F.pad(t, (0, w % 2, 0, h % 2)), 2, 2)
    elif wrong == "table_after_max":
        p = _act(F.max_pool2d(pool_src, 2, 2, ceil_mode=True), pool_tab)[0] * (gate if not k else 1.0)
    else:
        p = F.max_pool2d(t, 2, 2, ceil_mode=True)
    y = F.conv2d(torch.cat([v, p], 1), g["w3"].double()[:, :, None, None], _bias(g, "b3")).permute(0, 2, 3, 1).contiguous()
    return (y, pt, pu, pv, t) if parts else y


def border(h, w):
    m = torch.zeros(h, w, dtype=torch.bool)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    return m


_REFS = {}


def ref(name):
    """(inputs, float64 reference) of a case: computed once, shared by the tests, never modified."""
    if name not in _REFS:
        g = inputs(name)
        _REFS[name] = (g, reference(name, g))
    return _REFS[name]
