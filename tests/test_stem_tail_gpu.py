"""Direct C-ABI checks of lhn_stem_tail_fwd (depthwise K x K -> 1x1 -> 3x3 stride 2 | max pool -> 1x1 in one launch) against float64.

The arbiter is F.conv2d / F.max_pool2d(ceil_mode=True) in double (tests/stem_tail_cases.py); the yardstick is the launches it replaces
on the same inputs: lhn_conv_dw_fwd -> lhn_conv_pw_fwd -> lhn_conv_kxk_fwd (stride 2) -> lhn_maxpool2_fwd -> lhn_conv_pw_fwd through
buffers whose tables are tT, tU, tV (a bias the unfused depthwise / 3x3 kernel does not add rides in the table's shift, where the
plan puts it).  The fused result may be at most 3x as far from float64 as the unfused one, with the floor of test_bottleneck_gpu.py
(1e-4 of the output's peak).  Border pixels of y are compared on their own: that is where u must be padded with zeros, x with
zeros, and the pooling window clipped (tests/test_infer_fuse_stem_cpu.py shows on the CPU that each mistake is > 100 floors there)."""
import ctypes as C

import pytest
import torch

import stem_tail_cases as sc
from stem_tail_cases import CASES, C_OUT, FLOOR, M, PREFILL
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


def _with_bias(tab, bias, dev):
    """The [3][32] table that also adds `bias` ahead of the transform: scale * (v + b) + shift = scale * v + (shift + scale * b)."""
    if bias is None:
        return tab
    if tab is None:
        return torch.stack([torch.ones(M, device=dev), bias, torch.ones(M, device=dev)]).contiguous()
    out = tab.clone()
    out[1] += tab[0] * bias
    return out


def _run(name, g, dev, fused=True, scratch=True):
    c = CASES[name]
    n, h, w, k = c["n"], c["h"], c["w"], c["k"]
    oh, ow = (h + 1) // 2, (w + 1) // 2
    (xcs, xoff), (ycs, yoff) = c["x"], c["y"]
    L = _lib.lib()
    d = {key: v.to(dev) for key, v in g.items()}
    y = torch.full((n, oh, ow, ycs), PREFILL, device=dev)
    xv = _view(d["x"], xoff, M, d.get("xtab"), d.get("xgate"))
    yv = _view(y, yoff, C_OUT)
    st = _lib.stream()
    if fused:
        wt = torch.empty(9 * M * M, device=dev) if scratch else None
        _lib.check(L.lhn_stem_tail_fwd(C.byref(xv), k, _lib.ptr(d.get("w_dw")), _lib.ptr(d.get("bT")), _lib.ptr(d.get("tT")), _lib.ptr(d["w1"]),
                                       _lib.ptr(d.get("b1")), _lib.ptr(d.get("tU")), _lib.ptr(d["w2"]), _lib.ptr(d.get("b2")), _lib.ptr(d.get("tV")),
                                       _lib.ptr(d["w3"]), _lib.ptr(d.get("b3")), C.byref(yv), _lib.ptr(wt), st), "lhn_stem_tail_fwd")
    else:
        u, cat = torch.empty((n, h, w, M), device=dev), torch.empty((n, oh, ow, 2 * M), device=dev)
        if k:
            t = torch.empty((n, h, w, M), device=dev)
            _lib.check(L.lhn_conv_dw_fwd(C.byref(xv), _lib.ptr(d["w_dw"]), C.byref(_view(t, 0, M)), None, k, 1, k // 2, 1, None, st), "lhn_conv_dw_fwd")
            tv = _view(t, 0, M, _with_bias(d.get("tT"), d.get("bT"), dev))
        else:
            tv = xv
        _lib.check(L.lhn_conv_pw_fwd(C.byref(tv), _lib.ptr(d["w1"]), _lib.ptr(d.get("b1")), C.byref(_view(u, 0, M)), None, 1, None, None, st),
                   "lhn_conv_pw_fwd")
        _lib.check(L.lhn_conv_kxk_fwd(C.byref(_view(u, 0, M, d.get("tU"))), _lib.ptr(d["w2"]), C.byref(_view(cat, 0, M)), None, 2, None, None, st),
                   "lhn_conv_kxk_fwd")
        _lib.check(L.lhn_maxpool2_fwd(C.byref(tv), C.byref(_view(cat, M, M)), st), "lhn_maxpool2_fwd")
        # the table of the 64 channels: v's transform (with the 3x3's bias) | identity for the pooled half
        tv_ = _with_bias(d.get("tV"), d.get("b2"), dev)
        ctab = torch.stack([torch.ones(2 * M, device=dev), torch.zeros(2 * M, device=dev), torch.ones(2 * M, device=dev)]).contiguous()
        if tv_ is not None:
            ctab[:, :M] = tv_
        _lib.check(L.lhn_conv_pw_fwd(C.byref(_view(cat, 0, 2 * M, ctab)), _lib.ptr(d["w3"]), _lib.ptr(d.get("b3")), C.byref(yv), None, 1, None, None,
                                     st), "lhn_conv_pw_fwd")
    torch.cuda.synchronize()
    return y.cpu()


@pytest.mark.parametrize("name", list(CASES))
def test_stem_tail_matches_float64(dev, name):
    c = CASES[name]
    oh, ow, (ycs, yoff) = (c["h"] + 1) // 2, (c["w"] + 1) // 2, c["y"]
    g, ref = sc.ref(name)
    fused, five = _run(name, g, dev, True), _run(name, g, dev, False)
    peak = float(ref.abs().max())
    b = sc.border(oh, ow)
    rec = {}
    for region, mask in (("border", b), ("interior", ~b)):
        if not bool(mask.any()):
            continue
        r = ref[:, mask]
        e_f = float((fused[..., yoff:yoff + C_OUT].double()[:, mask] - r).abs().max()) / peak
        e_5 = float((five[..., yoff:yoff + C_OUT].double()[:, mask] - r).abs().max()) / peak
        rec[region] = (e_f, e_5, max(FLOOR, 3 * e_5))
        print(f"{name} {region}: fused {e_f:.3e} unfused {e_5:.3e} bar {max(FLOOR, 3 * e_5):.3e}")
    parity_record(f"stem_tail/{name}", **{f"{k}_{what}": v[i] for k, v in rec.items() for i, what in enumerate(("err_fused", "err_unfused", "bar"))})
    for region, (e_f, e_5, bar) in rec.items():
        assert e_f <= bar, (f"{name}: {region} pixels are {e_f:.3e} of the peak from float64 (unfused launches: {e_5:.3e}, bar {bar:.3e})" +
                            (" -- the border is where u and x are padded with zeros and the pooling window is clipped" if region == "border" else ""))
    if ycs > C_OUT:      # channels of y outside the view keep their prefill
        outside = torch.cat([fused[..., :yoff], fused[..., yoff + C_OUT:]], -1)
        assert bool((outside == PREFILL).all()), f"{name}: channels outside the output view were written"


@pytest.mark.parametrize("k", sc.KS)
@pytest.mark.parametrize("name", ["map_8x8", "map_37x19", "shift_far_12x70", "x_slice_256_table_gate", "all_null"])
def test_stem_tail_without_scratch(dev, name, k):
    """wt_scratch == NULL: the kernel reads the OIHW weights themselves -- the same products in the same order, so the same bits."""
    g, _ = sc.ref(f"{name}_k{k}")
    assert torch.equal(_run(f"{name}_k{k}", g, dev, scratch=False), _run(f"{name}_k{k}", g, dev, scratch=True))


@pytest.mark.parametrize("k", sc.KS)
@pytest.mark.parametrize("name", ["map_28x28", "map_9x70", "x_slice_256_table_gate", "mixed_sign"])
def test_stem_tail_repeats_bits(dev, name, k):
    g, _ = sc.ref(f"{name}_k{k}")
    a, b = _run(f"{name}_k{k}", g, dev), _run(f"{name}_k{k}", g, dev)
    assert torch.equal(a, b), f"{name}_k{k}: two calls on the same inputs differ"


@pytest.mark.parametrize("m,c,k,slope_in,overlap", [(64, 128, 3, None, False), (32, 64, 3, None, False), (64, 256, 0, None, False), (32, 128, 5, None, False),
                                                    (32, 128, 1, None, False), (32, 128, 3, ("tT", 2.0), False), (32, 128, 7, ("tU", 3.0), False),
                                                    (32, 128, 0, ("tV", 2.0), False), (32, 128, 0, ("x", 2.0), False), (32, 128, 3, ("tU", -0.5), False),
                                                    (32, 128, 3, None, True)])
def test_stem_tail_unsupported_shape(dev, m, c, k, slope_in, overlap):
    """Channel pairs and kernel sizes the kernel was not built for, the SiLU / relu-sigmoid sentinels in any table and y over x: the
    invalid-argument status with a message before any launch; neither y nor the weight scratch is written."""
    L = _lib.lib()
    x = torch.full((2, 8, 8, 256 if overlap else m), PREFILL, device=dev)
    y = x[:, :4, :4].contiguous() if overlap else torch.full((2, 4, 4, c), PREFILL, device=dev)
    kk = max(k, 1)
    w_dw, w1, w2, w3 = (sc._rand(s, 2 + j).to(dev) for j, s in enumerate(((m, 1, kk, kk), (m, m), (m, m, 3, 3), (c, 2 * m))))
    tabs = {key: torch.stack([torch.ones(ch), torch.zeros(ch), torch.full((ch,), 0.01)]).contiguous().to(dev) for key, ch in
            (("tT", m), ("tU", m), ("tV", m), ("x", x.shape[3]))}
    if slope_in is not None:
        tabs[slope_in[0]][2, 5] = slope_in[1]
    wt = torch.full((9 * m * m,), PREFILL, device=dev)
    xv = _view(x, 0, m, tabs["x"])
    if overlap:      # y as channels [0, 128) of a view over x's own memory (the kernel would read pixels it has already overwritten)
        yv = _view(x, 0, c)
        yv.H, yv.W = 4, 4
    else:
        yv = _view(y, 0, c)
    rc = L.lhn_stem_tail_fwd(C.byref(xv), k, _lib.ptr(w_dw), None, _lib.ptr(tabs["tT"]), _lib.ptr(w1), None, _lib.ptr(tabs["tU"]), _lib.ptr(w2), None,
                             _lib.ptr(tabs["tV"]), _lib.ptr(w3), None, C.byref(yv), _lib.ptr(wt), _lib.stream())
    torch.cuda.synchronize()
    assert rc != 0
    assert b"unsupported shape" in L.lhn_last_error(), L.lhn_last_error()
    assert bool((y == PREFILL).all()) and bool((x == PREFILL).all()) and bool((wt == PREFILL).all())
