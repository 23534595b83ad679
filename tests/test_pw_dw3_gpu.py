"""Direct C-ABI checks of lhn_conv_pw_dw3_fwd (1x1 -> pending transform -> depthwise 3x3 in one launch) against float64 torch.

The arbiter is F.conv2d in double; the yardstick is the two-launch path it replaces (lhn_conv_pw_fwd into a buffer whose table
is t_table, then lhn_conv_dw_fwd3) on the same inputs.  The fused result may be at most 3x as far from float64 as the
two-launch result (a different fp32 summation order, nothing worse), with the forward floor of test_model_gpu._check_block
(1e-4 of the output's peak).  Border pixels are compared on their own: the depthwise convolution pads t with zeros, and a
kernel that ran the 1x1 on a zero-padded x tile would put lrelu(shift1) there."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import parity_record
from litehandnet_amd import _lib
from litehandnet_amd._lib import View

pytestmark = pytest.mark.gpu
FLOOR = 1e-4
CM = 64

# name: n, h, w, x (cstride, coff), y (cstride, coff), slope1, shift1 offset, x table, x gate
CASES = {
    "bench_64_n64": (64, 64, 64, (64, 0), (64, 0), 0.01, 0.0, False, False),
    "bench_64": (2, 64, 64, (64, 0), (64, 0), 0.01, 0.0, False, False),
    "map_56": (2, 56, 56, (64, 0), (64, 0), 0.01, 0.0, False, False),
    "map_28": (3, 28, 28, (64, 0), (64, 0), 0.01, 0.0, False, False),
    "map_14": (3, 14, 14, (64, 0), (64, 0), 0.01, 0.0, False, False),
    "map_8": (5, 8, 8, (64, 0), (64, 0), 0.01, 0.0, False, False),
    "map_7": (3, 7, 7, (64, 0), (64, 0), 0.01, 0.0, False, False),
    "map_4": (3, 4, 4, (64, 0), (64, 0), 0.01, 0.5, False, False),
    "map_2x3": (3, 2, 3, (64, 0), (64, 0), 0.01, 0.5, False, False),
    "nonsquare_24x40": (2, 24, 40, (64, 0), (64, 0), 0.01, 0.0, False, False),
    "nonsquare_9x150": (1, 9, 150, (64, 0), (64, 0), 0.01, 0.0, False, False),
    "x_right_half_table": (2, 32, 32, (128, 64), (64, 0), 0.01, 0.0, True, False),
    "x_right_half_table_gate": (2, 64, 64, (128, 64), (64, 0), 0.01, 0.0, True, True),
    "y_right_half": (2, 64, 64, (64, 0), (128, 64), 0.01, 0.0, False, False),
    "both_halves_16": (2, 16, 16, (128, 64), (128, 64), 0.01, 0.0, True, True),
    "slope_0": (2, 32, 32, (64, 0), (64, 0), 0.0, 0.0, False, False),
    "slope_1": (2, 32, 32, (64, 0), (64, 0), 1.0, 0.0, False, False),
    "shift_far_64": (2, 64, 64, (64, 0), (64, 0), 0.01, 5.0, False, False),
    "shift_far_28_slope1": (2, 28, 28, (64, 0), (64, 0), 1.0, -4.0, False, False),
    "shift_far_8": (2, 8, 8, (128, 64), (128, 64), 0.01, 5.0, True, True),
    "shift_far_70": (1, 12, 70, (64, 0), (64, 0), 0.01, 3.0, False, False),
}
PREFILL = 7.0


def _rand(shape, seed, scale=1.0):
    return torch.from_numpy((np.random.Generator(np.random.PCG64(seed)).standard_normal(shape) * scale).astype(np.float32))


def _view(t, coff, c, table=None, gate=None):
    v = View()
    v.data, v.table, v.gate, v.pend = t.data_ptr(), (table.data_ptr() if table is not None else None), \
        (gate.data_ptr() if gate is not None else None), None
    v.N, v.H, v.W, v.cstride, v.coff, v.C = t.shape[0], t.shape[1], t.shape[2], t.shape[3], coff, c
    return v


def _inputs(name, seed=11):
    n, h, w, (xcs, xoff), _, slope1, shift_off, xtab, xgate = CASES[name]
    g = {"x": _rand((n, h, w, xcs), seed)}
    g["w1"] = _rand((CM, CM), seed + 1, CM ** -0.5)
    g["w2"] = _rand((CM, 1, 3, 3), seed + 2, 0.4)
    g["ttab"] = torch.stack([1 + 0.3 * _rand((CM,), seed + 3), 0.2 * _rand((CM,), seed + 4) + shift_off, torch.full((CM,), slope1)]).contiguous()
    if xtab:
        g["xtab"] = torch.stack([1 + 0.3 * _rand((xcs,), seed + 5), 0.2 * _rand((xcs,), seed + 6), torch.full((xcs,), 0.1)]).contiguous()
    if xgate:
        g["xgate"] = torch.sigmoid(_rand((n, xcs), seed + 7))
    return g


def _reference(name, g):
    """float64: the arithmetic of oracle/torch_ref.py (conv2d, per-channel affine, leaky_relu) on NCHW doubles."""
    _, _, _, (xcs, xoff), _, _, _, _, _ = CASES[name]
    x = g["x"].double()
    if "xtab" in g:
        t = g["xtab"].double()
        u = x * t[0] + t[1]
        x = torch.where(u > 0, u, u * t[2])
    if "xgate" in g:
        x = x * g["xgate"].double()[:, None, None, :]
    v = x[..., xoff:xoff + CM].permute(0, 3, 1, 2)
    tt = g["ttab"].double()
    u = F.conv2d(v, g["w1"].double()[:, :, None, None]) * tt[0][None, :, None, None] + tt[1][None, :, None, None]
    t = torch.where(u > 0, u, u * tt[2][None, :, None, None])
    y = F.conv2d(t, g["w2"].double(), padding=1, groups=CM)
    return y.permute(0, 2, 3, 1).contiguous()


def _run(name, g, dev, fused=True):
    n, h, w, (xcs, xoff), (ycs, yoff), _, _, _, _ = CASES[name]
    L = _lib.lib()
    d = {k: v.to(dev) for k, v in g.items()}
    y = torch.full((n, h, w, ycs), PREFILL, device=dev)
    xv = _view(d["x"], xoff, CM, d.get("xtab"), d.get("xgate"))
    yv = _view(y, yoff, CM)
    if fused:
        _lib.check(L.lhn_conv_pw_dw3_fwd(C.byref(xv), _lib.ptr(d["w1"]), _lib.ptr(d["ttab"]), _lib.ptr(d["w2"]), C.byref(yv), _lib.stream()),
                   "lhn_conv_pw_dw3_fwd")
    else:
        t = torch.empty((n, h, w, CM), device=dev)
        tv_out, tv_in = _view(t, 0, CM), _view(t, 0, CM, d["ttab"])
        _lib.check(L.lhn_conv_pw_fwd(C.byref(xv), _lib.ptr(d["w1"]), None, C.byref(tv_out), None, 1, None, None, _lib.stream()), "lhn_conv_pw_fwd")
        _lib.check(L.lhn_conv_dw_fwd3(C.byref(tv_in), _lib.ptr(d["w2"]), C.byref(yv), None, 3, 1, 1, 1, None, None, None, None, _lib.stream()),
                   "lhn_conv_dw_fwd3")
    torch.cuda.synchronize()
    return y.cpu()


def _border(h, w):
    m = torch.zeros(h, w, dtype=torch.bool)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    return m


@pytest.mark.parametrize("name", list(CASES))
def test_pw_dw3_matches_float64(dev, name):
    n, h, w, _, (ycs, yoff), _, _, _, _ = CASES[name]
    g = _inputs(name)
    ref = _reference(name, g)
    fused, two = _run(name, g, dev, True), _run(name, g, dev, False)
    peak = float(ref.abs().max())
    b = _border(h, w)
    rec = {}
    for region, mask in (("border", b), ("interior", ~b)):
        if not bool(mask.any()):
            continue
        r = ref[:, mask]
        e_f = float((fused[..., yoff:yoff + CM].double()[:, mask] - r).abs().max()) / peak
        e_t = float((two[..., yoff:yoff + CM].double()[:, mask] - r).abs().max()) / peak
        rec[region] = (e_f, e_t, max(FLOOR, 3 * e_t))
        print(f"{name} {region}: fused {e_f:.3e} two-launch {e_t:.3e} bar {max(FLOOR, 3 * e_t):.3e}")
    parity_record(f"pw_dw3/{name}", **{f"{k}_{what}": v[i] for k, v in rec.items() for i, what in enumerate(("err_fused", "err_two_launch", "bar"))})
    for region, (e_f, e_t, bar) in rec.items():
        assert e_f <= bar, (f"{name}: {region} pixels are {e_f:.3e} of the peak from float64 (two launches: {e_t:.3e}, bar {bar:.3e})" +
                            (" -- the border is where t must be padded with zeros, not with lrelu(shift1)" if region == "border" else ""))
    if ycs > CM:      # channels of y outside the view keep their bits
        outside = torch.cat([fused[..., :yoff], fused[..., yoff + CM:]], -1)
        assert bool((outside == PREFILL).all()), f"{name}: channels outside the output view were written"


@pytest.mark.parametrize("name", ["bench_64", "map_14", "x_right_half_table_gate", "nonsquare_9x150"])
def test_pw_dw3_repeats_bits(dev, name):
    g = _inputs(name)
    a, b = _run(name, g, dev), _run(name, g, dev)
    assert torch.equal(a, b), f"{name}: two calls on the same inputs differ"


@pytest.mark.parametrize("cin,cm", [(32, 32), (64, 32), (128, 128), (40, 40)])
def test_pw_dw3_unsupported_shape(dev, cin, cm):
    """Channel counts the kernel was not built for: the invalid-argument status with a message, and y is not written."""
    L = _lib.lib()
    x = _rand((2, 16, 16, cin), 1).to(dev)
    y = torch.full((2, 16, 16, cm), PREFILL, device=dev)
    w1, w2, tt = _rand((cm, cin), 2).to(dev), _rand((cm, 1, 3, 3), 3).to(dev), torch.ones(3, cm, device=dev)
    xv, yv = _view(x, 0, cin), _view(y, 0, cm)
    rc = L.lhn_conv_pw_dw3_fwd(C.byref(xv), _lib.ptr(w1), _lib.ptr(tt), _lib.ptr(w2), C.byref(yv), _lib.stream())
    torch.cuda.synchronize()
    assert rc != 0
    assert b"unsupported shape" in L.lhn_last_error()
    assert bool((y == PREFILL).all())
