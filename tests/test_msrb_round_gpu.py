"""Direct C-ABI checks of lhn_msrb_round_fwd (both dilated depthwise 3x3 branches of an MSRB round and the pooling of its attention
in one pass) against float64 torch.

The arbiter is F.conv2d / adaptive_avg_pool2d in double; the yardstick is the three-launch path it replaces on the same inputs
(lhn_conv_dw_fwd3 twice into the halves of y, then lhn_avgpool_fwd).  Per region (border pixels and interior on their own: the
convolutions pad the VALUE of x with zeros, which "shift far" tables make visible) the fused y may be at most 3x as far from
float64 as the three-launch y, with the forward floor of test_model_gpu._check_block (1e-4 of the reference's peak).  The pooled
means are held to the same rule with the error normalised by the peak of the float64 FEATURE MAP: a pooled entry is a mean of
map values, so its error cannot exceed the map's.  Constant-map cases pin the bin membership: n ones summed and divided by n
is exactly 1.0 in fp32, one pixel too many or too few in a bin is not."""
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


def _case(n, h, w, half=64, oh=3, x0=None, x1=None, extra=None, xtab=None, xgate=False, y=None, ytab=False, const=False):
    """x0, x1: (buffer "a" | "b", cstride, coff) of the two input views (default: the halves of one 2 * half buffer); extra: None or
    coef2, the extras then are the halves of a gated buffer with a table; xtab: None | "near" | a shift offset ("shift far");
    y: (cstride, coff); oh: 0 (pooled NULL) | 1 | 3; ytab: a non-trivial y.table with slope 1; const: the constant-map inputs."""
    return dict(n=n, h=h, w=w, half=half, oh=oh, x0=x0 or ("a", 2 * half, 0), x1=x1 or ("a", 2 * half, half), extra=extra, xtab=xtab,
                xgate=xgate, y=y or (2 * half, 0), ytab=ytab, const=const)


CASES = {f"half{_h}_16": _case(2, 16, 16, _h, ytab=True) for _h in (32, 64, 128)}
CASES.update({
    "map_64": _case(2, 64, 64, ytab=True),
    "map_56": _case(2, 56, 56),                  # three-way bins of 19 / 20 rows with one-pixel overlaps
    "map_16_se": _case(3, 16, 16, oh=1, ytab=True),
    "map_8": _case(3, 8, 8, ytab=True),
    "map_7": _case(3, 7, 7),
    "map_4": _case(3, 4, 4, ytab=True),
    "map_2x3": _case(3, 2, 3, ytab=True),        # smaller than 3: every pixel sits in several bins; most dilation-2 taps fall outside
    "map_1x5": _case(3, 1, 5, half=32),
    "map_1x5_se": _case(2, 1, 5, half=32, oh=1),
    "nonsquare_24x40": _case(2, 24, 40, ytab=True),
    "nonsquare_9x150": _case(1, 9, 150, half=32),
    "two_buffers": _case(2, 16, 16, x0=("a", 128, 32), x1=("b", 192, 128), xtab="near", xgate=True, ytab=True),
    "two_buffers_64": _case(1, 64, 64, half=32, x0=("a", 64, 32), x1=("b", 96, 0), xtab="near", xgate=True),
    "one_buffer_slices": _case(2, 24, 40, half=32, x0=("a", 128, 64), x1=("a", 128, 0), xtab="near", xgate=True),
    "extra_1_1": _case(2, 32, 32, extra=(1.0, 1.0), xtab="near", xgate=True, ytab=True),
    "extra_half_2": _case(2, 16, 16, half=32, extra=(0.5, 2.0), xtab="near", ytab=True),
    "extra_two_buffers_56": _case(1, 56, 56, half=32, extra=(1.0, 1.0), x0=("a", 64, 0), x1=("b", 64, 32), xgate=True),
    "shift_far_64": _case(1, 64, 64, half=32, xtab=5.0),
    "shift_far_16": _case(2, 16, 16, xtab=-4.0, ytab=True),
    "shift_far_7_extra_none": _case(2, 7, 7, half=32, xtab=4.5, xgate=True),
    "shift_far_extra_24x40": _case(1, 24, 40, half=32, extra=(1.0, 1.0), xtab=-5.0),
    "y_slice_128_of_192": _case(2, 16, 16, y=(192, 64), ytab=True),
    "y_slice_64_of_128_se": _case(2, 32, 32, half=32, y=(128, 32), oh=1),
    "pooled_null": _case(2, 16, 16, oh=0),
    "pooled_null_56_extra": _case(1, 56, 56, half=32, oh=0, extra=(1.0, 1.0)),
    "ytab_null_se": _case(2, 8, 8, half=32, oh=1),
    # Multi-item: 520 images x 4 channel groups = 2,080 work items, more than one resident round of workgroups (at most 256 CUs x 2
    # resident x 2 = 1,024 blocks in the persistent grid), so every block walks several items with a different image each.
    "multi_item_n520_16": _case(520, 16, 16, ytab=True),
    "const_64": _case(2, 64, 64, const=True),
    "const_56": _case(2, 56, 56, half=32, const=True),
    "const_7": _case(2, 7, 7, const=True),
    "const_2x3": _case(2, 2, 3, half=32, const=True),
    "const_16_se": _case(2, 16, 16, half=32, oh=1, const=True),
})


def _rand(shape, seed, scale=1.0):
    return torch.from_numpy((np.random.Generator(np.random.PCG64(seed)).standard_normal(shape) * scale).astype(np.float32))


def _view(t, coff, c, table=None, gate=None):
    v = View()
    v.data, v.table, v.gate, v.pend = t.data_ptr(), (table.data_ptr() if table is not None else None), \
        (gate.data_ptr() if gate is not None else None), None
    v.N, v.H, v.W, v.cstride, v.coff, v.C = t.shape[0], t.shape[1], t.shape[2], t.shape[3], coff, c
    return v


def _table(cs, seed, shift, slope):
    return torch.stack([1 + 0.3 * _rand((cs,), seed), 0.2 * _rand((cs,), seed + 1) + shift, torch.full((cs,), slope)]).contiguous()


def _inputs(name, seed=17):
    c = CASES[name]
    n, h, w, half = c["n"], c["h"], c["w"], c["half"]
    g = {}
    for j, (buf, cs, _) in enumerate((c["x0"], c["x1"])):
        if "x" + buf in g:
            continue
        g["x" + buf] = torch.ones(n, h, w, cs) if c["const"] else _rand((n, h, w, cs), seed + 10 * j)
        if c["xtab"] is not None:
            g["xtab" + buf] = _table(cs, seed + 10 * j + 1, 0.0 if c["xtab"] == "near" else float(c["xtab"]), 0.1)
        if c["xgate"]:
            g["xgate" + buf] = torch.sigmoid(_rand((n, cs), seed + 10 * j + 3))
    if c["const"]:
        wc = torch.zeros(half, 1, 3, 3)
        wc[:, :, 1, 1] = 1.0
        g["w1"], g["w2"] = wc, wc.clone()
    else:
        g["w1"], g["w2"] = _rand((half, 1, 3, 3), seed + 30, 0.4), _rand((half, 1, 3, 3), seed + 31, 0.4)
    if c["extra"] is not None:
        g["e"] = _rand((n, h, w, 2 * half), seed + 40)
        g["etab"] = _table(2 * half, seed + 41, 0.0, 0.1)
        g["egate"] = torch.sigmoid(_rand((n, 2 * half), seed + 43))
    if c["ytab"]:
        g["ytab"] = _table(c["y"][0], seed + 50, 0.3, 1.0)
    return g


def _value(x, tab, gate):
    x = x.double()
    if tab is not None:
        u = x * tab.double()[0] + tab.double()[1]
        x = torch.where(u > 0, u, u * tab.double()[2])
    if gate is not None:
        x = x * gate.double()[:, None, None, :]
    return x


def _reference(name, g):
    """float64 (raw y [N,H,W,C], pooled [N,OH,OW,C] or None): the arithmetic of oracle/torch_ref.py on NCHW doubles."""
    c = CASES[name]
    half, ys = c["half"], []
    for k, (buf, _, coff) in enumerate((c["x0"], c["x1"])):
        v = _value(g["x" + buf], g.get("xtab" + buf), g.get("xgate" + buf))[..., coff:coff + half]
        if c["extra"] is not None:
            e = _value(g["e"], g["etab"], g["egate"])[..., k * half:(k + 1) * half]
            v = c["extra"][0] * v + c["extra"][1] * e
        d = k + 1
        ys.append(F.conv2d(v.permute(0, 3, 1, 2), g["w1" if k == 0 else "w2"].double(), padding=d, dilation=d, groups=half))
    y = torch.cat(ys, 1)
    pooled = None
    if c["oh"]:
        z = y
        if "ytab" in g:
            t = g["ytab"].double()[:, c["y"][1]:c["y"][1] + 2 * half]
            z = y * t[0][None, :, None, None] + t[1][None, :, None, None]       # (slope 1)
        pooled = F.adaptive_avg_pool2d(z, c["oh"]).permute(0, 2, 3, 1).contiguous()
    return y.permute(0, 2, 3, 1).contiguous(), pooled


_REFS = {}


def _ref(name):
    """(inputs, float64 references) of a case: computed once, shared by the tests, never modified."""
    if name not in _REFS:
        g = _inputs(name)
        _REFS[name] = (g, _reference(name, g))
    return _REFS[name]


def _run(name, g, dev, fused=True, ytab=True):
    """(y buffer, pooled or None) on the CPU.  ytab=False: the same call with y.table NULL."""
    c = CASES[name]
    n, h, w, half, oh = c["n"], c["h"], c["w"], c["half"], c["oh"]
    ycs, yoff = c["y"]
    L = _lib.lib()
    d = {k: v.to(dev) for k, v in g.items()}
    y = torch.full((n, h, w, ycs), PREFILL, device=dev)
    pooled = torch.full((n, oh, oh, 2 * half), PREFILL, device=dev) if oh else None
    xs = (View * 2)(*[_view(d["x" + buf], coff, half, d.get("xtab" + buf), d.get("xgate" + buf)) for buf, _, coff in (c["x0"], c["x1"])])
    es = (View * 2)(*[_view(d["e"], k * half, half, d["etab"], d["egate"]) for k in range(2)]) if c["extra"] is not None else None
    coef = (C.c_float * 2)(*c["extra"]) if c["extra"] is not None else None
    yt = d.get("ytab") if ytab else None
    if fused:
        nbytes = L.lhn_msrb_round_scratch_bytes(n, h, w, 2 * half)
        assert nbytes > 0
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        yv = _view(y, yoff, 2 * half, yt)
        _lib.check(L.lhn_msrb_round_fwd(xs, es, coef, _lib.ptr(d["w1"]), _lib.ptr(d["w2"]), C.byref(yv), _lib.ptr(pooled), oh, oh,
                                        _lib.ptr(scratch), _lib.stream()), "lhn_msrb_round_fwd")
    else:
        for k in range(2):
            yk = _view(y, yoff + k * half, half)
            _lib.check(L.lhn_conv_dw_fwd3(C.byref(xs[k]), _lib.ptr(d["w1" if k == 0 else "w2"]), C.byref(yk), None, 3, 1, k + 1, k + 1, None,
                                          C.byref(es[k]) if es is not None else None, coef, None, _lib.stream()), "lhn_conv_dw_fwd3")
        if oh:
            yv = _view(y, yoff, 2 * half, yt)
            _lib.check(L.lhn_avgpool_fwd(C.byref(yv), _lib.ptr(pooled), oh, oh, _lib.stream()), "lhn_avgpool_fwd")
    torch.cuda.synchronize()
    return y.cpu(), (pooled.cpu() if oh else None)


def _border(h, w):
    m = torch.zeros(h, w, dtype=torch.bool)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    return m


def test_case_table_and_reference_cpu_side():
    """The case table covers what it must and no reference is degenerate (no GPU work: runs first, cheaply)."""
    cs = CASES.values()
    assert {32, 64, 128} <= {c["half"] for c in cs if (c["h"], c["w"]) == (16, 16)}
    assert {(64, 64), (56, 56), (16, 16), (8, 8), (7, 7)} <= {(c["h"], c["w"]) for c in cs if c["half"] == 64 and not c["const"]}
    assert {(4, 4), (2, 3), (1, 5), (24, 40), (9, 150)} <= {(c["h"], c["w"]) for c in cs}
    assert any(c["x0"][0] != c["x1"][0] and c["x0"][1:] != c["x1"][1:] and c["xtab"] and c["xgate"] for c in cs)
    assert any(c["x0"][0] == c["x1"][0] and c["x0"][1] > 2 * c["half"] for c in cs)
    assert {(1.0, 1.0), (0.5, 2.0)} <= {c["extra"] for c in cs if c["extra"] is not None}
    assert any(isinstance(c["xtab"], float) and abs(c["xtab"]) >= 4 for c in cs)
    assert any(c["y"][0] > 2 * c["half"] for c in cs)
    assert {0, 1, 3} <= {c["oh"] for c in cs} and {True, False} <= {c["ytab"] for c in cs if c["oh"]}
    assert {(64, 64), (56, 56), (7, 7), (2, 3)} <= {(c["h"], c["w"]) for c in cs if c["const"]}
    assert sum(c["n"] > 3 for c in cs) == 1
    for name, c in CASES.items():
        for buf, xcs, coff in (c["x0"], c["x1"]):
            assert coff + c["half"] <= xcs, name
        assert c["y"][1] + 2 * c["half"] <= c["y"][0], name
        if c["extra"] is not None:
            assert c["w"] >= 16, name          # the three-launch yardstick takes a second source from 16 columns on (dilation 2)
        if c["n"] > 3:
            continue
        g, (ref, pref) = _ref(name)
        assert ref.shape == (c["n"], c["h"], c["w"], 2 * c["half"]) and bool(torch.isfinite(ref).all())
        assert float(ref.abs().max()) > 0.1 and float((ref != 0).float().mean()) > 0.99, name
        if c["oh"]:
            assert pref.shape == (c["n"], c["oh"], c["oh"], 2 * c["half"]) and bool(torch.isfinite(pref).all())
            assert float(pref.abs().max()) > 0, name
        if c["const"]:
            assert bool((ref == 1).all()) and bool((pref == 1).all()), name


@pytest.mark.parametrize("name", [k for k, c in CASES.items() if not c["const"]])
def test_msrb_round_matches_float64(dev, name):
    c = CASES[name]
    h, w, half, (ycs, yoff) = c["h"], c["w"], c["half"], c["y"]
    g, (ref, pref) = _ref(name)
    (fused, fp), (three, tp) = _run(name, g, dev, True), _run(name, g, dev, False)
    peak = float(ref.abs().max())
    b = _border(h, w)
    rec = {}
    for region, mask in (("border", b), ("interior", ~b)):
        if not bool(mask.any()):
            continue
        r = ref[:, mask]
        e_f = float((fused[..., yoff:yoff + 2 * half].double()[:, mask] - r).abs().max()) / peak
        e_t = float((three[..., yoff:yoff + 2 * half].double()[:, mask] - r).abs().max()) / peak
        rec[region] = (e_f, e_t, max(FLOOR, 3 * e_t))
    if c["oh"]:
        if "ytab" in g:          # the map the pooled means are means of: the consumed value
            t = g["ytab"].double()[:, yoff:yoff + 2 * half]
            peak_map = min(peak, float((ref * t[0] + t[1]).abs().max()))      # (never a larger yardstick than the raw map's peak)
        else:
            peak_map = peak
        e_f, e_t = float((fp.double() - pref).abs().max()) / peak_map, float((tp.double() - pref).abs().max()) / peak_map
        rec["pooled"] = (e_f, e_t, max(FLOOR, 3 * e_t))
    for region, (e_f, e_t, bar) in rec.items():
        print(f"{name} {region}: fused {e_f:.3e} three-launch {e_t:.3e} bar {bar:.3e}")
    parity_record(f"msrb_round/{name}", **{f"{k}_{what}": v[i] for k, v in rec.items() for i, what in enumerate(("err_fused", "err_three_launch", "bar"))})
    for region, (e_f, e_t, bar) in rec.items():
        assert e_f <= bar, (f"{name}: {region} is {e_f:.3e} of the peak from float64 (three launches: {e_t:.3e}, bar {bar:.3e})" +
                            (" -- the border is where value(x) must be padded with zeros, not with lrelu(shift_x)" if region == "border" else ""))
    if ycs > 2 * half:      # channels of y outside the view keep their bits
        outside = torch.cat([fused[..., :yoff], fused[..., yoff + 2 * half:]], -1)
        assert bool((outside == PREFILL).all()), f"{name}: channels outside the output view were written"
    if c["oh"] and "ytab" in g:      # the table changes the pooled means and leaves the raw y alone
        plain, pp = _run(name, g, dev, True, ytab=False)
        assert torch.equal(plain, fused), f"{name}: y.table changed the raw output"
        assert not torch.equal(pp, fp), f"{name}: y.table did not reach the pooled means"


@pytest.mark.parametrize("name", [k for k, c in CASES.items() if c["const"]])
def test_msrb_round_constant_map_pools_to_exactly_one(dev, name):
    c = CASES[name]
    g, (ref, pref) = _ref(name)
    y, pooled = _run(name, g, dev)
    assert bool((y == 1.0).all()), f"{name}: the centre tap of a map of ones is not 1 everywhere"
    bad = (pooled != 1.0).nonzero()
    assert bad.numel() == 0, f"{name}: pooled[{bad[0].tolist()}] = {float(pooled[tuple(bad[0])])!r}: a bin holds the wrong pixels"


@pytest.mark.parametrize("name", ["map_64", "map_56", "two_buffers", "extra_1_1", "nonsquare_9x150"])
def test_msrb_round_repeats_bits(dev, name):
    g, _ = _ref(name)
    (a, pa), (b, pb) = _run(name, g, dev), _run(name, g, dev)
    assert torch.equal(a, b) and torch.equal(pa, pb), f"{name}: two calls on the same inputs differ"


@pytest.mark.parametrize("what", ["half16", "half40", "oh2", "oh3_ow1", "no_scratch", "y_over_x1"])
def test_msrb_round_unsupported_shape(dev, what):
    """Shapes the entry point was not built for: the invalid-argument status with a message, and neither y nor pooled is written."""
    L = _lib.lib()
    half = {"half16": 16, "half40": 40}.get(what, 32)
    oh, ow = {"oh2": (2, 2), "oh3_ow1": (3, 1)}.get(what, (3, 3))
    x = torch.full((2, 16, 16, 4 * half), PREFILL, device=dev)
    y = x if what == "y_over_x1" else torch.full((2, 16, 16, 2 * half), PREFILL, device=dev)
    pooled = torch.full((2, 3, 3, 2 * half), PREFILL, device=dev)
    scratch = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    w1, w2 = _rand((half, 1, 3, 3), 2).to(dev), _rand((half, 1, 3, 3), 3).to(dev)
    xs = (View * 2)(_view(x, 0, half), _view(x, half, half))
    yv = _view(y, (half + 4 if what == "y_over_x1" else 0), 2 * half)      # y over x[1] only: channels [half + 4, 3 * half + 4)
    assert L.lhn_msrb_round_scratch_bytes(2, 16, 16, 2 * half) == (0 if what in ("half16", "half40") else 2 * 2 * 1 * 9 * 2 * half * 4)
    rc = L.lhn_msrb_round_fwd(xs, None, None, _lib.ptr(w1), _lib.ptr(w2), C.byref(yv), _lib.ptr(pooled), oh, ow,
                              None if what == "no_scratch" else _lib.ptr(scratch), _lib.stream())
    torch.cuda.synchronize()
    assert rc != 0
    assert b"unsupported shape" in L.lhn_last_error()
    assert bool((y == PREFILL).all()) and bool((pooled == PREFILL).all())
