"""Direct C-ABI checks of lhn_bottleneck_fwd at C = 256, Cm in {64, 128} against float64 torch, the way tests/test_bottleneck_gpu.py
checks C = 128.

The arbiter is F.conv2d in double (tests/bottleneck256_cases.py); the yardstick is the four-launch path the fused launch replaces on
the same inputs: lhn_conv_pw_fwd -> lhn_conv_kxk_fwd -> lhn_conv_pw_fwd -> lhn_ew_fwd through three intermediate buffers whose
tables are t1, t2, t3.  The fused result may be at most 3x as far from float64 as the four-launch result, with the project's forward
floor (1e-4 of the output's peak).  Border pixels are judged on their own: the 3x3 pads t1 with zeros, and a kernel that padded
with act1(shift1) would be > 100 floors off there in the "shift far" cases (tests/test_infer_fuse_bneck256_cpu.py shows it)."""
import ctypes as C

import pytest
import torch

import bottleneck256_cases as bc
from bottleneck256_cases import CASES, C_IO, FLOOR, PREFILL
from conftest import parity_record
from litehandnet_amd import _lib
from litehandnet_amd._lib import View

pytestmark = pytest.mark.gpu


def _view(t, coff, c, table=None, gate=None):
    v = View()
    v.data, v.table, v.gate, v.pend = t.data_ptr(), (table.data_ptr() if table is not None else None), \
        (gate.data_ptr() if gate is not None else None), None
    v.N, v.H, v.W, v.cstride, v.coff, v.C = t.shape[0], t.shape[1], t.shape[2], t.shape[3], coff, c
    return v


def _run(name, g, dev, fused=True, scratch=True):
    c = CASES[name]
    n, h, w, cm = c["n"], c["h"], c["w"], c["cm"]
    (xcs, xoff), (ycs, yoff) = c["x"], c["y"]
    L = _lib.lib()
    d = {k: v.to(dev) for k, v in g.items()}
    y = torch.full((n, h, w, ycs), PREFILL, device=dev)
    xv = _view(d["x"], xoff, C_IO, d.get("xtab"), d.get("xgate"))
    yv = _view(y, yoff, C_IO)
    st = _lib.stream()
    if fused:
        wt = torch.empty(9 * cm * cm, device=dev) if scratch else None
        _lib.check(L.lhn_bottleneck_fwd(C.byref(xv), cm, _lib.ptr(d["w1"]), _lib.ptr(d.get("b1")), _lib.ptr(d.get("t1")), _lib.ptr(d["w2"]),
                                        _lib.ptr(d.get("t2")), _lib.ptr(d["w3"]), _lib.ptr(d.get("b3")), _lib.ptr(d.get("t3")),
                                        c["out_slope"], C.byref(yv), _lib.ptr(wt), st), "lhn_bottleneck_fwd")
    else:
        a, b, e = (torch.empty((n, h, w, ch), device=dev) for ch in (cm, cm, C_IO))
        _lib.check(L.lhn_conv_pw_fwd(C.byref(xv), _lib.ptr(d["w1"]), _lib.ptr(d.get("b1")), C.byref(_view(a, 0, cm)), None, 1, None, None, st),
                   "lhn_conv_pw_fwd")
        _lib.check(L.lhn_conv_kxk_fwd(C.byref(_view(a, 0, cm, d.get("t1"))), _lib.ptr(d["w2"]), C.byref(_view(b, 0, cm)), None, 1, None, None, st),
                   "lhn_conv_kxk_fwd")
        _lib.check(L.lhn_conv_pw_fwd(C.byref(_view(b, 0, cm, d.get("t2"))), _lib.ptr(d["w3"]), _lib.ptr(d.get("b3")), C.byref(_view(e, 0, C_IO)), None,
                                     1, None, None, st), "lhn_conv_pw_fwd")
        srcs = (View * 2)(xv, _view(e, 0, C_IO, d.get("t3")))
        _lib.check(L.lhn_ew_fwd(srcs, 2, C.byref(yv), C.c_float(c["out_slope"]), st), "lhn_ew_fwd")
    torch.cuda.synchronize()
    return y.cpu()


@pytest.mark.parametrize("name", list(CASES))
def test_bottleneck256_matches_float64(dev, name):
    c = CASES[name]
    h, w, (ycs, yoff) = c["h"], c["w"], c["y"]
    g, ref = bc.ref(name)
    fused, four = _run(name, g, dev, True), _run(name, g, dev, False)
    peak = float(ref.abs().max())
    b = bc.border(h, w)
    rec = {}
    for region, mask in (("border", b), ("interior", ~b)):
        if not bool(mask.any()):
            continue
        r = ref[:, mask]
        e_f = float((fused[..., yoff:yoff + C_IO].double()[:, mask] - r).abs().max()) / peak
        e_4 = float((four[..., yoff:yoff + C_IO].double()[:, mask] - r).abs().max()) / peak
        rec[region] = (e_f, e_4, max(FLOOR, 3 * e_4))
        print(f"{name} {region}: fused {e_f:.3e} four-launch {e_4:.3e} bar {max(FLOOR, 3 * e_4):.3e}")
    parity_record(f"bneck256/{name}", **{f"{k}_{what}": v[i] for k, v in rec.items() for i, what in enumerate(("err_fused", "err_four_launch", "bar"))})
    for region, (e_f, e_4, bar) in rec.items():
        assert e_f <= bar, (f"{name}: {region} pixels are {e_f:.3e} of the peak from float64 (four launches: {e_4:.3e}, bar {bar:.3e})" +
                            (" -- the border is where t1 must be padded with zeros, not with act1(shift1)" if region == "border" else ""))
    if ycs > C_IO:      # channels of y outside the view keep their prefill
        outside = torch.cat([fused[..., :yoff], fused[..., yoff + C_IO:]], -1)
        assert bool((outside == PREFILL).all()), f"{name}: channels outside the output view were written"


@pytest.mark.parametrize("name", ["map_8x8_m64", "map_8x8_m128", "shift_far_12x70_m64", "shift_far_12x70_m128", "both_slices_m128", "all_null_m64"])
def test_bottleneck256_without_scratch(dev, name):
    """wt_scratch == NULL: the kernel reads the OIHW weights themselves -- the same products in the same order, so the same bits."""
    g, _ = bc.ref(name)
    assert torch.equal(_run(name, g, dev, scratch=False), _run(name, g, dev, scratch=True))


@pytest.mark.parametrize("name", ["const_9x11_m64", "const_9x11_m128"])
def test_constant_input_closed_form_256(dev, name):
    """y = lrelu_out((-1)^c * (1 + taps / 9)).  In each of the three sums every term has the same sign (condition number 1), so the
    standard bound of a length-n fp32 sum in any order, n * 2^-24 relative, carries through the stages additively: the bar is
    (256 + 9 Cm + Cm + 4) * 2^-24 of the peak -- the three sum lengths (the first one 256 long, whatever the K chunks) plus the
    rounding of 1 / (9 Cm), the residual add and the slope."""
    cm = CASES[name]["cm"]
    g, _ = bc.ref(name)
    want = bc.const_answer(name)
    got = _run(name, g, dev).double()
    err = float((got - want).abs().max()) / float(want.abs().max())
    bar = (256 + 9 * cm + cm + 4) * 2.0 ** -24
    print(f"{name}: closed form {err:.3e} bar {bar:.3e}")
    parity_record(f"bneck256/{name}_closed_form", rel_err=err, bar=bar)
    assert err <= bar, (err, bar)


@pytest.mark.parametrize("name", ["map_16x16_m64", "map_14x14_m128", "x_slice_512_table_gate_m128", "map_9x70_m64"])
def test_bottleneck256_repeats_bits(dev, name):
    g, _ = bc.ref(name)
    a, b = _run(name, g, dev), _run(name, g, dev)
    assert torch.equal(a, b), f"{name}: two calls on the same inputs differ"


@pytest.mark.parametrize("c,cm,yc,out_slope,overlap", [(256, 32, 256, 0.01, False), (256, 256, 256, 0.01, False), (192, 64, 192, 0.01, False),
                                                       (256, 64, 128, 0.01, False), (256, 64, 256, 2.0, False), (256, 128, 256, 0.01, True)])
def test_bottleneck256_unsupported_shape(dev, c, cm, yc, out_slope, overlap):
    """Channel pairs the kernel was not built for, y.C != x.C, the SiLU sentinel as output slope and y over x: the invalid-argument
    status with "unsupported shape" before any launch; neither y nor the weight scratch is written."""
    L = _lib.lib()
    x = torch.full((2, 8, 8, 512 if overlap else c), PREFILL, device=dev)
    y = x if overlap else torch.full((2, 8, 8, yc), PREFILL, device=dev)
    w1, w2, w3 = (bc._rand(s, 2 + j).to(dev) for j, s in enumerate(((cm, c), (cm, cm, 3, 3), (c, cm))))
    wt = torch.full((9 * cm * cm,), PREFILL, device=dev)
    xv, yv = _view(x, 0, c), _view(y, 128 if overlap else 0, yc)
    rc = L.lhn_bottleneck_fwd(C.byref(xv), cm, _lib.ptr(w1), None, None, _lib.ptr(w2), None, _lib.ptr(w3), None, None, out_slope, C.byref(yv),
                              _lib.ptr(wt), _lib.stream())
    torch.cuda.synchronize()
    assert rc != 0
    assert b"unsupported shape" in L.lhn_last_error()
    assert bool((y == PREFILL).all()) and bool((wt == PREFILL).all())
