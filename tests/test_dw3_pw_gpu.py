"""Direct C-ABI checks of lhn_conv_dw3_pw_fwd (depthwise 3x3 -> pending transform -> 1x1 in one launch) against float64 torch.

The arbiter is F.conv2d in double; the yardstick is the two-launch path it replaces (lhn_conv_dw_fwd3 into a buffer whose table
is t_table, then lhn_conv_pw_fwd) on the same inputs.  The fused result may be at most 3x as far from float64 as the two-launch
result (a different fp32 summation order, nothing worse), with the forward floor of test_model_gpu._check_block (1e-4 of the
output's peak).  Border pixels are compared on their own: the depthwise convolution pads the VALUE of x with zeros, and a kernel
that transformed a zero-padded raw tile would put lrelu(shift_x) there ("shift far" cases make that visible)."""
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
PREFILL = 7.0


def _case(n, h, w, cin=64, cout=64, dil=1, x=None, y=None, slope=0.01, ttab=True, bias=True, xtab=None, xgate=False):
    """x, y: (cstride, coff) of the views (default: the whole buffer); xtab: None | "near" | a shift offset ("shift far")."""
    return dict(n=n, h=h, w=w, cin=cin, cout=cout, dil=dil, x=x or (cin, 0), y=y or (cout, 0), slope=slope, ttab=ttab, bias=bias,
                xtab=xtab, xgate=xgate)


CASES = {}
for _ci, _co in ((64, 32), (32, 32), (64, 64)):
    for _d in (1, 2):
        CASES[f"c{_ci}_{_co}_d{_d}_16"] = _case(2, 16, 16, _ci, _co, _d)
CASES.update({
    "map_64": _case(2, 64, 64, 64, 64, 1),
    "map_64_d2_c32": _case(2, 64, 64, 64, 32, 2),
    "map_56": _case(2, 56, 56, 32, 32, 1),
    "map_28_d2": _case(3, 28, 28, 64, 64, 2),
    "map_14": _case(3, 14, 14, 64, 32, 1),
    "map_8": _case(5, 8, 8, 32, 32, 2),
    "map_7": _case(3, 7, 7, 64, 64, 1),
    "map_4_d2": _case(3, 4, 4, 64, 32, 2),
    "map_2x3_d2": _case(3, 2, 3, 32, 32, 2),
    "map_1x5_d2": _case(3, 1, 5, 64, 64, 2),
    "nonsquare_24x40": _case(2, 24, 40, 64, 64, 2),
    "nonsquare_9x150": _case(1, 9, 150, 64, 32, 1),
    "nonsquare_9x150_d2": _case(1, 9, 150, 32, 32, 2),
    "x_slice_128_table_gate": _case(2, 32, 32, 64, 64, 1, x=(128, 64), xtab="near", xgate=True),
    "x_slice_64_table_gate": _case(2, 16, 16, 32, 32, 2, x=(64, 32), xtab="near", xgate=True),
    "y_slice_32_of_64": _case(2, 32, 32, 32, 32, 1, y=(64, 32)),
    "y_slice_64_of_128": _case(2, 64, 64, 64, 64, 2, y=(128, 64)),
    "both_slices_16": _case(2, 16, 16, 64, 64, 1, x=(128, 64), y=(128, 64), xtab="near", xgate=True),
    "ttab_null": _case(2, 32, 32, 64, 32, 1, ttab=False),
    "ttab_null_bias_null": _case(2, 16, 16, 32, 32, 2, ttab=False, bias=False),
    "slope_0": _case(2, 32, 32, 64, 64, 1, slope=0.0),
    "slope_1_bias_null": _case(2, 32, 32, 64, 64, 2, slope=1.0, bias=False),
    "shift_far_64": _case(2, 64, 64, 64, 64, 1, xtab=5.0),
    "shift_far_28_d2": _case(2, 28, 28, 64, 32, 2, xtab=-4.0),
    "shift_far_8": _case(2, 8, 8, 32, 32, 2, x=(64, 32), xtab=5.0, xgate=True),
    "shift_far_12x70": _case(1, 12, 70, 64, 64, 2, xtab=4.0),
    # Multi-item: the launcher asks for one resident round of workgroups (CUs x resident workgroups per CU, at most 256 x 2 = 512 on
    # this device) and cuts each image into bands of at least 8 rows only while images x strips stays below that.  520 single-strip
    # images exceed it, so every workgroup owns a whole 16 x 16 image and walks it in 16 / RPS + 2 * DIL / RPS = 5 steps of RPS = 4
    # rows (the ring of RPS + 2 * DIL = 8 rows wraps twice), and the 520 workgroups are more than one resident round.
    "multi_item_n520_16_d2": _case(520, 16, 16, 64, 32, 2),
})


def _rand(shape, seed, scale=1.0):
    return torch.from_numpy((np.random.Generator(np.random.PCG64(seed)).standard_normal(shape) * scale).astype(np.float32))


def _view(t, coff, c, table=None, gate=None):
    v = View()
    v.data, v.table, v.gate, v.pend = t.data_ptr(), (table.data_ptr() if table is not None else None), \
        (gate.data_ptr() if gate is not None else None), None
    v.N, v.H, v.W, v.cstride, v.coff, v.C = t.shape[0], t.shape[1], t.shape[2], t.shape[3], coff, c
    return v


def _inputs(name, seed=11):
    c = CASES[name]
    cin, cout, xcs = c["cin"], c["cout"], c["x"][0]
    g = {"x": _rand((c["n"], c["h"], c["w"], xcs), seed)}
    g["wd"] = _rand((cin, 1, 3, 3), seed + 1, 0.4)
    g["wp"] = _rand((cout, cin), seed + 2, cin ** -0.5)
    if c["ttab"]:
        g["ttab"] = torch.stack([1 + 0.3 * _rand((cin,), seed + 3), 0.2 * _rand((cin,), seed + 4), torch.full((cin,), c["slope"])]).contiguous()
    if c["bias"]:
        g["bias"] = 0.5 * _rand((cout,), seed + 8)
    if c["xtab"] is not None:
        off = 0.0 if c["xtab"] == "near" else float(c["xtab"])
        g["xtab"] = torch.stack([1 + 0.3 * _rand((xcs,), seed + 5), 0.2 * _rand((xcs,), seed + 6) + off, torch.full((xcs,), 0.1)]).contiguous()
    if c["xgate"]:
        g["xgate"] = torch.sigmoid(_rand((c["n"], xcs), seed + 7))
    return g


def _reference(name, g):
    """float64: the arithmetic of oracle/torch_ref.py (conv2d, per-channel affine, leaky_relu) on NCHW doubles."""
    c = CASES[name]
    cin, xoff, dil = c["cin"], c["x"][1], c["dil"]
    x = g["x"].double()
    if "xtab" in g:
        t = g["xtab"].double()
        u = x * t[0] + t[1]
        x = torch.where(u > 0, u, u * t[2])
    if "xgate" in g:
        x = x * g["xgate"].double()[:, None, None, :]
    v = x[..., xoff:xoff + cin].permute(0, 3, 1, 2)
    u = F.conv2d(v, g["wd"].double(), padding=dil, dilation=dil, groups=cin)
    if "ttab" in g:
        tt = g["ttab"].double()
        u = u * tt[0][None, :, None, None] + tt[1][None, :, None, None]
        u = torch.where(u > 0, u, u * tt[2][None, :, None, None])
    y = F.conv2d(u, g["wp"].double()[:, :, None, None], g["bias"].double() if "bias" in g else None)
    return y.permute(0, 2, 3, 1).contiguous()


_REFS = {}


def _ref(name):
    """(inputs, float64 reference) of a case: computed once, shared by the tests, never modified."""
    if name not in _REFS:
        g = _inputs(name)
        _REFS[name] = (g, _reference(name, g))
    return _REFS[name]


def _run(name, g, dev, fused=True):
    c = CASES[name]
    n, h, w, cin, cout, dil = c["n"], c["h"], c["w"], c["cin"], c["cout"], c["dil"]
    (xcs, xoff), (ycs, yoff) = c["x"], c["y"]
    L = _lib.lib()
    d = {k: v.to(dev) for k, v in g.items()}
    y = torch.full((n, h, w, ycs), PREFILL, device=dev)
    xv = _view(d["x"], xoff, cin, d.get("xtab"), d.get("xgate"))
    yv = _view(y, yoff, cout)
    if fused:
        _lib.check(L.lhn_conv_dw3_pw_fwd(C.byref(xv), _lib.ptr(d["wd"]), dil, _lib.ptr(d.get("ttab")), _lib.ptr(d["wp"]), _lib.ptr(d.get("bias")),
                                         C.byref(yv), _lib.stream()), "lhn_conv_dw3_pw_fwd")
    else:
        t = torch.empty((n, h, w, cin), device=dev)
        tv_out, tv_in = _view(t, 0, cin), _view(t, 0, cin, d.get("ttab"))
        _lib.check(L.lhn_conv_dw_fwd3(C.byref(xv), _lib.ptr(d["wd"]), C.byref(tv_out), None, 3, 1, dil, dil, None, None, None, None, _lib.stream()),
                   "lhn_conv_dw_fwd3")
        _lib.check(L.lhn_conv_pw_fwd(C.byref(tv_in), _lib.ptr(d["wp"]), _lib.ptr(d.get("bias")), C.byref(yv), None, 1, None, None, _lib.stream()),
                   "lhn_conv_pw_fwd")
    torch.cuda.synchronize()
    return y.cpu()


def _border(h, w):
    m = torch.zeros(h, w, dtype=torch.bool)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    return m


def test_case_table_and_reference_cpu_side():
    """The case table covers what it must and no reference is degenerate (no GPU work: runs first, cheaply)."""
    combos = {(c["cin"], c["cout"], c["dil"]) for k, c in CASES.items() if (c["h"], c["w"]) == (16, 16)}
    assert {(a, b, d) for a, b in ((64, 32), (32, 32), (64, 64)) for d in (1, 2)} <= combos
    sizes = {(c["h"], c["w"]) for c in CASES.values()}
    assert {(64, 64), (56, 56), (28, 28), (14, 14), (8, 8), (7, 7), (4, 4), (2, 3), (1, 5), (24, 40), (9, 150), (12, 70)} <= sizes
    for name, c in CASES.items():
        assert c["n"] <= 5 or name.startswith("multi_item"), name
        if c["h"] <= 4 and c["w"] <= 5:                               # most taps fall outside
            assert c["dil"] == 2, name
        assert c["x"][1] + c["cin"] <= c["x"][0] and c["y"][1] + c["cout"] <= c["y"][0], name
        if c["n"] > 5:
            continue
        g, ref = _ref(name)
        assert ref.shape == (c["n"], c["h"], c["w"], c["cout"]) and bool(torch.isfinite(ref).all())
        assert float(ref.abs().max()) > 0.1 and float((ref != 0).float().mean()) > 0.99, name


@pytest.mark.parametrize("name", list(CASES))
def test_dw3_pw_matches_float64(dev, name):
    c = CASES[name]
    h, w, cout, (ycs, yoff) = c["h"], c["w"], c["cout"], c["y"]
    g, ref = _ref(name)
    fused, two = _run(name, g, dev, True), _run(name, g, dev, False)
    peak = float(ref.abs().max())
    b = _border(h, w)
    rec = {}
    for region, mask in (("border", b), ("interior", ~b)):
        if not bool(mask.any()):
            continue
        r = ref[:, mask]
        e_f = float((fused[..., yoff:yoff + cout].double()[:, mask] - r).abs().max()) / peak
        e_t = float((two[..., yoff:yoff + cout].double()[:, mask] - r).abs().max()) / peak
        rec[region] = (e_f, e_t, max(FLOOR, 3 * e_t))
        print(f"{name} {region}: fused {e_f:.3e} two-launch {e_t:.3e} bar {max(FLOOR, 3 * e_t):.3e}")
    parity_record(f"dw3_pw/{name}", **{f"{k}_{what}": v[i] for k, v in rec.items() for i, what in enumerate(("err_fused", "err_two_launch", "bar"))})
    for region, (e_f, e_t, bar) in rec.items():
        assert e_f <= bar, (f"{name}: {region} pixels are {e_f:.3e} of the peak from float64 (two launches: {e_t:.3e}, bar {bar:.3e})" +
                            (" -- the border is where value(x) must be padded with zeros, not with lrelu(shift_x)" if region == "border" else ""))
    if ycs > cout:      # channels of y outside the view keep their bits
        outside = torch.cat([fused[..., :yoff], fused[..., yoff + cout:]], -1)
        assert bool((outside == PREFILL).all()), f"{name}: channels outside the output view were written"


@pytest.mark.parametrize("name", ["map_64", "map_14", "x_slice_128_table_gate", "nonsquare_9x150_d2"])
def test_dw3_pw_repeats_bits(dev, name):
    g, _ = _ref(name)
    a, b = _run(name, g, dev), _run(name, g, dev)
    assert torch.equal(a, b), f"{name}: two calls on the same inputs differ"


@pytest.mark.parametrize("cin,cout,dil,overlap", [(128, 128, 1, False), (40, 40, 1, False), (64, 128, 1, False), (16, 32, 1, False),
                                                  (64, 64, 3, False), (64, 64, 1, True)])
def test_dw3_pw_unsupported_shape(dev, cin, cout, dil, overlap):
    """Channel counts / dilations the kernel was not built for, and y over x: the invalid-argument status with a message, and y
    is not written."""
    L = _lib.lib()
    x = torch.full((2, 16, 16, 128 if overlap else cin), PREFILL, device=dev)
    y = x if overlap else torch.full((2, 16, 16, cout), PREFILL, device=dev)
    wd, wp, tt = _rand((cin, 1, 3, 3), 2).to(dev), _rand((cout, cin), 3).to(dev), torch.ones(3, cin, device=dev)
    xv, yv = _view(x, 0, cin), _view(y, 32 if overlap else 0, cout)
    rc = L.lhn_conv_dw3_pw_fwd(C.byref(xv), _lib.ptr(wd), dil, _lib.ptr(tt), _lib.ptr(wp), None, C.byref(yv), _lib.stream())
    torch.cuda.synchronize()
    assert rc != 0
    assert b"unsupported shape" in L.lhn_last_error()
    assert bool((y == PREFILL).all())
