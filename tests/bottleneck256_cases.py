"""Case table, inputs and float64 reference of lhn_bottleneck_fwd at C = 256, Cm in {64, 128} (tests/test_bottleneck256_gpu.py runs
them on the GPU, tests/test_infer_fuse_bneck256_cpu.py checks on the CPU that no case is degenerate).  Importable without a GPU and
without liblhn.so.  The arithmetic, the case dictionary and the helpers are those of tests/bottleneck_cases.py (C = 128); what is
new at this width is that the kernel runs its first 1x1 over K chunks of x (two of 128 channels at Cm = 64, four of 64 at Cm = 128),
its second 1x1 over two output feature tiles per wave, and, at Cm = 128, its 3x3 with two pixel tiles per wave and t2 over the head
of t1 in LDS.  The shapes are the smallest at which tiling (1x5 .. 24x40: below, at and above one 8 x 8 tile, ragged in both
directions), the halo (every map), the K chunks (every case: all 256 channels carry independent random data) and the channel
slices (a 512-wide buffer) can each go wrong."""
import numpy as np
import torch
import torch.nn.functional as F

from bottleneck_cases import FLOOR, PREFILL, _act, _alt, _rand, border  # noqa: F401  (re-exported for the tests)

C_IO = 256
MIDS = (64, 128)


def _case(n, h, w, cm, x=None, y=None, tabs=(True, True, True), biases=(True, True), slopes=(0.01, 0.01, 1.0), out_slope=0.01,
          shift_far=False, xtab=False, xgate=False, const=False):
    """The fields of bottleneck_cases._case; the default views are the whole 256-channel buffer."""
    return dict(n=n, h=h, w=w, cm=cm, x=x or (C_IO, 0), y=y or (C_IO, 0), tabs=tuple(tabs), biases=tuple(biases), slopes=tuple(slopes),
                out_slope=out_slope, shift_far=shift_far, xtab=xtab, xgate=xgate, const=const)


CASES = {}
for _cm in MIDS:
    for _n, _h, _w in ((5, 1, 5), (5, 2, 3), (4, 4, 4), (3, 7, 7), (3, 8, 8), (2, 14, 14), (2, 16, 16), (2, 9, 70), (2, 24, 40)):
        CASES[f"map_{_h}x{_w}_m{_cm}"] = _case(_n, _h, _w, _cm)
    CASES.update({
        f"x_slice_512_table_gate_m{_cm}": _case(2, 16, 16, _cm, x=(512, 128), xtab=True, xgate=True),
        f"y_slice_512_m{_cm}": _case(2, 16, 16, _cm, y=(512, 256)),
        f"both_slices_m{_cm}": _case(2, 14, 14, _cm, x=(512, 256), y=(512, 64), xtab=True, xgate=True),
        f"t1_null_m{_cm}": _case(2, 8, 8, _cm, tabs=(False, True, True)),
        f"t2_null_m{_cm}": _case(2, 8, 8, _cm, tabs=(True, False, True)),
        f"t3_null_m{_cm}": _case(2, 8, 8, _cm, tabs=(True, True, False)),
        f"b1_null_m{_cm}": _case(2, 8, 8, _cm, biases=(False, True)),
        f"b3_null_m{_cm}": _case(2, 8, 8, _cm, biases=(True, False)),
        f"all_null_m{_cm}": _case(2, 7, 7, _cm, tabs=(False, False, False), biases=(False, False)),
        f"out_slope_0_m{_cm}": _case(2, 8, 8, _cm, out_slope=0.0),
        f"out_slope_1_m{_cm}": _case(2, 8, 8, _cm, out_slope=1.0),
        f"mid_slopes_0_m{_cm}": _case(2, 14, 14, _cm, slopes=(0.0, 0.0, 1.0)),
        f"mid_slopes_1_m{_cm}": _case(2, 14, 14, _cm, slopes=(1.0, 1.0, 1.0)),
        f"shift_far_8_m{_cm}": _case(2, 8, 8, _cm, shift_far=True),
        f"shift_far_12x70_m{_cm}": _case(1, 12, 70, _cm, shift_far=True),
        f"const_9x11_m{_cm}": _case(2, 9, 11, _cm, tabs=(False, False, False), biases=(False, False), const=True),
    })
    # Multi-round: the launcher's work item is one 8 x 8 output tile of one image = one workgroup, and both instantiations keep TWO
    # workgroups resident on a CU (80,000 B of LDS each of 163,840 B; 192 / 256 registers per lane = 2 waves per SIMD), so one
    # resident round is 2 x 256 CUs = 512 workgroups.  520 images of 4 x 4 are 520 tiles: more than one round.
    CASES[f"multi_round_n520_4_m{_cm}"] = _case(520, 4, 4, _cm)


def inputs(name, seed=41):
    """CPU float32 tensors of a case: x [N,H,W,xcs], w1, w2, w3 and, where the case has them, b1, b3, t1, t2, t3, xtab, xgate."""
    c = CASES[name]
    cm, xcs = c["cm"], c["x"][0]
    if c["const"]:
        # every pixel the same: x[c] = (-1)^c, w1[m][c] = (-1)^(m+c) / 256, w2[o][i][tap] = (-1)^(o+i) / (9 Cm), w3[c][m] = (-1)^(c+m) / Cm
        x = _alt(xcs).expand(c["n"], c["h"], c["w"], xcs).contiguous()
        return {"x": x, "w1": (_alt(cm)[:, None] * _alt(C_IO)[None, :] / C_IO).contiguous(),
                "w2": (_alt(cm)[:, None, None, None] * _alt(cm)[None, :, None, None] / (9.0 * cm)).expand(cm, cm, 3, 3).contiguous(),
                "w3": (_alt(C_IO)[:, None] * _alt(cm)[None, :] / cm).contiguous()}
    g = {"x": _rand((c["n"], c["h"], c["w"], xcs), seed),
         "w1": _rand((cm, C_IO), seed + 1, C_IO ** -0.5),
         "w2": _rand((cm, cm, 3, 3), seed + 2, (9 * cm) ** -0.5 * 1.5),
         "w3": _rand((C_IO, cm), seed + 3, cm ** -0.5 * 1.5)}
    if c["biases"][0]:
        g["b1"] = 0.3 * _rand((cm,), seed + 4)
    if c["biases"][1]:
        g["b3"] = 0.3 * _rand((C_IO,), seed + 5)
    for j, (k, ch) in enumerate((("t1", cm), ("t2", cm), ("t3", C_IO))):
        if c["tabs"][j]:
            shift = 0.2 * _rand((ch,), seed + 7 + 2 * j)
            if k == "t1" and c["shift_far"]:
                u = np.random.Generator(np.random.PCG64(seed + 20)).uniform(4.0, 5.0, ch).astype(np.float32)
                shift = torch.from_numpy(u) * _alt(ch)
            g[k] = torch.stack([1 + 0.3 * _rand((ch,), seed + 6 + 2 * j), shift, torch.full((ch,), float(c["slopes"][j]))]).contiguous()
    if c["xtab"]:
        g["xtab"] = torch.stack([1 + 0.3 * _rand((xcs,), seed + 12), 0.2 * _rand((xcs,), seed + 13), torch.full((xcs,), 0.1)]).contiguous()
    if c["xgate"]:
        g["xgate"] = torch.sigmoid(_rand((c["n"], xcs), seed + 14))
    return g


def reference(name, g, wrong_padding=False, parts=False):
    """float64 NHWC result (F.conv2d on NCHW doubles).  parts=True: also the pre-activation tensors of t1, t2 and of the final sum.
    wrong_padding=True: t1 padded with act1(shift1) instead of zeros (see bottleneck_cases.reference)."""
    c = CASES[name]
    xoff = c["x"][1]
    x = g["x"].double()
    if "xtab" in g:
        t = g["xtab"].double()
        u = x * t[0] + t[1]
        x = torch.where(u > 0, u, u * t[2])
    if "xgate" in g:
        x = x * g["xgate"].double()[:, None, None, :]
    v = x[..., xoff:xoff + C_IO].permute(0, 3, 1, 2)
    t1, p1 = _act(F.conv2d(v, g["w1"].double()[:, :, None, None], g["b1"].double() if "b1" in g else None), g.get("t1"))
    if wrong_padding:
        pad = _act(torch.zeros(1, c["cm"], 1, 1, dtype=torch.float64), g.get("t1"))[0]
        u2 = F.conv2d(F.pad(t1 - pad, (1, 1, 1, 1)) + pad, g["w2"].double())
    else:
        u2 = F.conv2d(t1, g["w2"].double(), padding=1)
    t2, p2 = _act(u2, g.get("t2"))
    t3, _ = _act(F.conv2d(t2, g["w3"].double()[:, :, None, None], g["b3"].double() if "b3" in g else None), g.get("t3"))
    s = v + t3
    y = torch.where(s > 0, s, s * c["out_slope"]).permute(0, 2, 3, 1).contiguous()
    return (y, p1, p2, s) if parts else y


def const_answer(name):
    """Closed form of a const case: y[n, h, w, c] = lrelu_out((-1)^c * (1 + taps(h, w) / 9)), taps = the 3x3 taps inside the map."""
    c = CASES[name]
    th = torch.tensor([3.0 - (i == 0) - (i == c["h"] - 1) for i in range(c["h"])], dtype=torch.float64)
    tw = torch.tensor([3.0 - (j == 0) - (j == c["w"] - 1) for j in range(c["w"])], dtype=torch.float64)
    s = (1.0 + th[:, None] * tw[None, :] / 9.0)[None, :, :, None] * _alt(C_IO).double()[None, None, None, :]
    s = s.expand(c["n"], c["h"], c["w"], C_IO)
    return torch.where(s > 0, s, s * c["out_slope"]).contiguous()


_REFS = {}


def ref(name):
    """(inputs, float64 reference) of a case: computed once, shared by the tests, never modified."""
    if name not in _REFS:
        g = inputs(name)
        _REFS[name] = (g, reference(name, g))
    return _REFS[name]
