"""Direct C-ABI checks of the four grouped ConditionalChannelWeighting entry points (lhn_ccw_pool_fwd, lhn_ccw_gate_fwd, lhn_ccw_dw_fwd,
lhn_ccw_shuffle_fwd) against float64 torch (tests/ccw_cases.py).

The arbiter is float64; the yardstick is the launch chain each call replaces, on the same inputs.  Per output the fused result may
be at most 3x as far from float64 as that chain, with the forward floor of test_msrb_round_gpu (1e-4 of the float64 peak); border
pixels and interior are judged on their own (the depthwise convolution pads the PRODUCT with zeros, which "shift far" tables make
visible).  Constant-map cases are exact in fp32: a pixel in the wrong window, a wrong gate cell or a mixed-up sample is a bit
difference there, not a tolerance question."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import ccw_cases as cc
from ccw_cases import CASES, FLOOR, PREFILL
from conftest import parity_record
from litehandnet_amd import _lib
from litehandnet_amd._lib import CcwSe, View

pytestmark = pytest.mark.gpu

_RUNS = {}


def _runs(name, dev):
    """(Device, fused outputs, chain outputs) of a case: run once, shared by the tests, never modified."""
    if name not in _RUNS:
        g, r = cc.ref(name)
        D = cc.Device(name, g, r, dev)
        f = cc.run_fused(D)
        _RUNS[name] = (D, f, cc.run_chain(D, f["y_dev"]))
    return _RUNS[name]


def _border(h, w):
    m = torch.zeros(h, w, dtype=torch.bool)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    return m


def _judge(rec, tag, fused, chain, ref64):
    """Border and interior of one output on their own: (error of the fused call, of the chain, bar), of the float64 peak."""
    peak = float(ref64.abs().max())
    b = _border(ref64.shape[1], ref64.shape[2])
    for region, mask in (("border", b), ("interior", ~b)):
        if not bool(mask.any()):
            continue
        e_f = float((fused.double()[:, mask] - ref64[:, mask]).abs().max()) / peak
        e_c = float((chain.double()[:, mask] - ref64[:, mask]).abs().max()) / peak
        rec[f"{tag}_{region}"] = (e_f, e_c, max(FLOOR, 3 * e_c))


def test_case_table_cpu_side():
    """The case table covers what it must, and its references are sound (no GPU work)."""
    cs = CASES.values()
    assert {2, 3} <= {c["n"] for c in cs} and {2, 3, 4} == {len(c["maps"]) for c in cs}
    assert any(c["maps"] == [(16, 16), (8, 8)] and c["chans"] == [20, 40] for c in cs)
    assert any(c["maps"] == [(16, 16), (8, 8), (4, 4)] for c in cs)
    assert any(c["maps"] == [(16, 16), (8, 8), (4, 4), (2, 2)] and max(c["chans"]) == 160 for c in cs)
    assert any(c["maps"][-1] == (1, 1) and c["maps"][0] != (1, 1) for c in cs) and any(c["maps"] == [(12, 20), (6, 10)] for c in cs)
    assert any(len(set(c["maps"])) == 1 and c["maps"][0] != (1, 1) for c in cs)
    assert any(c["wide"] and not c["const"] for c in cs) and any(c["xtab"] == "neg" for c in cs) and any(c["xgate"] for c in cs)
    assert any(isinstance(c["xtab"], float) and abs(c["xtab"]) >= 4 for c in cs) and sum(c["const"] for c in cs) >= 2
    cc.check_reference()


@pytest.mark.parametrize("name", [k for k, c in CASES.items() if not c["const"]])
def test_ccw_calls_match_float64(dev, name):
    c = CASES[name]
    g, r = cc.ref(name)
    D, f, ch = _runs(name, dev)
    rec = {}
    _judge(rec, "pooled", f["pooled"], ch["pooled"], r["pooled"])
    _judge(rec, "g", f["g"], ch["g"], r["g"])
    for b, cb in enumerate(c["chans"]):
        oy, oo = D.lay[b][4], D.lay[b][6]
        _judge(rec, f"y{b}", f["y"][b][..., oy:oy + cb], ch["y"][b][..., oy:oy + cb], r["y"][b])
        out64, _ = cc.shuffle_reference(name, g, b, f["y"][b][..., oy:oy + cb])
        _judge(rec, f"out{b}", f["out"][b][..., oo:oo + 2 * cb], ch["out"][b][..., oo:oo + 2 * cb], out64)
    for k, (e_f, e_c, bar) in rec.items():
        print(f"{name} {k}: fused {e_f:.3e} chain {e_c:.3e} bar {bar:.3e}")
    parity_record(f"ccw/{name}", **{f"{k}_{what}": v[i] for k, v in rec.items() for i, what in enumerate(("err_fused", "err_chain", "bar"))})
    for k, (e_f, e_c, bar) in rec.items():
        assert e_f <= bar, (f"{name}: {k} is {e_f:.3e} of the peak from float64 (the chain it replaces: {e_c:.3e}, bar {bar:.3e})" +
                            (" -- the border is where the PRODUCT must be padded with zeros" if k.endswith("border") else ""))
    # floats outside every output keep their bits: channels outside the views, the scratch behind its end
    for b, cb in enumerate(c["chans"]):
        for t, off, width in ((f["y"][b], D.lay[b][4], cb), (f["out"][b], D.lay[b][6], 2 * cb)):
            outside = torch.cat([t[..., :off], t[..., off + width:]], -1)
            assert bool((outside == PREFILL).all()), f"{name}: branch {b}: channels outside an output view were written"
    assert bool((f["scratch"][-64:] == PREFILL).all()) and bool((f["scratch"][:-64] != PREFILL).all()), f"{name}: scratch extent"


@pytest.mark.parametrize("name", [k for k, c in CASES.items() if c["const"]])
def test_ccw_constant_maps_are_exact(dev, name):
    c = CASES[name]
    g, r = cc.ref(name)
    D, f, _ = _runs(name, dev)
    bad = (f["pooled"].double() != r["pooled"]).nonzero()
    assert bad.numel() == 0, f"{name}: pooled[{bad[0].tolist()}] = {float(f['pooled'][tuple(bad[0])])!r}: a window holds the wrong pixels"
    for b, cb in enumerate(c["chans"]):
        oy, oo, o1 = D.lay[b][4], D.lay[b][6], D.lay[b][1]
        y = f["y"][b][..., oy:oy + cb]
        bad = (y.double() != r["y"][b]).nonzero()
        assert bad.numel() == 0, (f"{name}: y[{b}][{bad[0].tolist()}] = {float(y[tuple(bad[0])])!r}, expected "
                                  f"{float(r['y'][b][tuple(bad[0])])!r}: a wrong gate cell, sample or padding")
        assert torch.equal(f["out"][b][..., oo:oo + 2 * cb:2], g[f"x{b}"][..., o1:o1 + cb]), f"{name}: out[{b}][2j] is not x1[j]"


@pytest.mark.parametrize("name", ["b4_stage4_at_64", "nonsquare_12x20", "gated_input", "ratio_8"])
def test_ccw_calls_repeat_bits(dev, name):
    D, f, _ = _runs(name, dev)
    again = cc.run_fused(D)
    assert torch.equal(again["pooled"], f["pooled"]) and torch.equal(again["g"], f["g"]) and torch.equal(again["scratch"], f["scratch"])
    assert all(torch.equal(a, b) for k in ("y", "out") for a, b in zip(again[k], f[k])), f"{name}: two calls on the same inputs differ"


def test_gate_differs_per_sample(dev):
    """A mix-up of n: both results sit far closer to their float64 reference than to the one computed with the samples' gates
    exchanged -- and the exchange is visible, which it would not be if the samples' gates were alike."""
    name = "per_sample_gates"
    c = CASES[name]
    g, r = cc.ref(name)
    D, f, _ = _runs(name, dev)
    off = 0
    for b, ((h, w), cb) in enumerate(zip(c["maps"], c["chans"])):
        oy, oo, o2 = D.lay[b][4], D.lay[b][6], D.lay[b][2]
        y = f["y"][b][..., oy:oy + cb]
        v2 = cc.value(g[f"x{b}"], None, None)[..., o2:o2 + cb].permute(0, 3, 1, 2)
        up = F.interpolate(r["g_in"].double().flip(0)[..., off:off + cb].permute(0, 3, 1, 2), size=(h, w), mode="nearest")
        off += cb
        y_swapped = F.conv2d(v2 * up, g[f"wdw{b}"].double(), padding=1, groups=cb).permute(0, 2, 3, 1)
        peak = float(r["y"][b].abs().max())
        d_true, d_swap = float((y.double() - r["y"][b]).abs().max()) / peak, float((y.double() - y_swapped).abs().max()) / peak
        assert d_swap > 30 * FLOOR and d_true < 0.01 * d_swap, (b, d_true, d_swap)      # (ten times the bar of 3 x FLOOR: a mix-up would fail)
        out64, (p1, p2) = cc.shuffle_reference(name, g, b, y)
        t = g[f"ytab{b}"].double()[:, oy:oy + cb]
        swapped = out64.clone()
        swapped[..., 1::2] = (y.double() * t[0] + t[1]) * cc.relu_sigmoid(p2).flip(0)[:, None, None, :]
        got, peak = f["out"][b][..., oo:oo + 2 * cb].double(), float(out64.abs().max())
        d_true, d_swap = float((got - out64).abs().max()) / peak, float((got - swapped).abs().max()) / peak
        assert d_swap > 30 * FLOOR and d_true < 0.01 * d_swap, (b, d_true, d_swap)      # (ten times the bar of 3 x FLOOR: a mix-up would fail)


REFUSALS = ["B1", "B5", "ratio", "order", "empty_view", "C164", "C_odd", "y_over_x2", "out_over_x1", "out_over_y", "no_scratch", "J0"]


@pytest.mark.parametrize("what", REFUSALS)
def test_ccw_unsupported_shape(dev, what):
    """Each refusal returns the invalid-argument status with its message before any launch: nothing is written."""
    L = _lib.lib()
    n = 2
    maps = {"ratio": [(12, 12), (8, 8)], "order": [(8, 8), (16, 16), (8, 8)]}.get(what, [(16, 16), (8, 8)])
    chans = {"C164": [164, 40], "C_odd": [20, 42], "order": [20, 40, 80]}.get(what, [20, 40])
    if what == "B5":
        maps, chans = [(16, 16)] * 4 + [(8, 8)], [20] * 5
    B = 1 if what == "B1" else len(maps)
    hm, wm = maps[-1]
    x = [torch.full((n, h, w, 2 * cb), PREFILL, device=dev) for (h, w), cb in zip(maps, chans)]
    y = [torch.full((n, h, w, cb), PREFILL, device=dev) for (h, w), cb in zip(maps, chans)]
    out = [torch.full((n, h, w, 2 * cb), PREFILL, device=dev) for (h, w), cb in zip(maps, chans)]
    pooled, gate = (torch.full((n, hm, wm, sum(chans)), PREFILL, device=dev) for _ in range(2))
    scratch = torch.full((1 << 18,), PREFILL, device=dev)
    nb = len(maps)
    x1 = (View * nb)(*[cc.view(t, 0, cb) for t, cb in zip(x, chans)])
    x2 = (View * nb)(*[cc.view(t, cb, cb) for t, cb in zip(x, chans)])
    yv = (View * nb)(*[cc.view(t, 0, cb) for t, cb in zip(y, chans)])
    ov = (View * nb)(*[cc.view(t, 0, 2 * cb) for t, cb in zip(out, chans)])
    H, W, Cs = ((C.c_int * nb)(*v) for v in ([m[0] for m in maps], [m[1] for m in maps], chans))
    if what == "empty_view":                                   # a view nobody filled in: all zeros
        x2[1], yv[1] = View(), View()
        H[1] = W[1] = 0
    if what == "y_over_x2":
        yv[0] = cc.view(x[0], chans[0] - 4, chans[0])          # y[0] over the last 4 channels of x1 and most of x2
    if what == "out_over_x1":
        ov[1] = cc.view(x[1], 0, 2 * chans[1])
    if what == "out_over_y":
        big = torch.full((n,) + maps[0] + (2 * chans[0],), PREFILL, device=dev)
        yv[0], ov[0] = cc.view(big, 0, chans[0]), cc.view(big, 0, 2 * chans[0])
        y[0] = big
    ws = (C.c_void_p * nb)(*[torch.ones(cb, 1, 3, 3, device=dev).data_ptr() for cb in chans])
    keep = [torch.ones(cb * cb, device=dev) for cb in chans]
    ses = (CcwSe * nb)()
    for b, cb in enumerate(chans):
        ses[b].w1 = ses[b].b1 = ses[b].w2 = ses[b].b2 = keep[b].data_ptr()
        ses[b].J = 0 if what == "J0" else cb // 4
    sp = None if what == "no_scratch" else _lib.ptr(scratch)
    st = _lib.stream()
    only_shuffle = what in ("out_over_x1", "out_over_y", "J0")
    only_scratch = what in ("no_scratch", "y_over_x2") or only_shuffle
    if not only_scratch:
        assert L.lhn_ccw_scratch_bytes(n, B, H, W, Cs) == 0
    calls = {"pool": lambda: L.lhn_ccw_pool_fwd(x2, B, _lib.ptr(pooled), st),
             "dw": lambda: L.lhn_ccw_dw_fwd(x2, B, _lib.ptr(gate), ws, yv, sp, st),
             "shuffle": lambda: L.lhn_ccw_shuffle_fwd(x1, yv, B, ses, sp, ov, st)}
    if only_shuffle:
        del calls["pool"], calls["dw"]
    elif only_scratch:
        del calls["pool"]
        if what == "y_over_x2":
            del calls["shuffle"]
    for k, call in calls.items():
        rc = call()
        torch.cuda.synchronize()
        assert rc == 1, (what, k, rc)
        assert b"unsupported shape" in L.lhn_last_error(), (what, k, L.lhn_last_error())
    for t in x + y + out + [pooled, scratch]:
        assert bool((t == PREFILL).all()), f"{what}: a refused call wrote something"


@pytest.mark.parametrize("what", ["Ct324", "mid41"])
def test_ccw_gate_unsupported_shape(dev, what):
    L = _lib.lib()
    Ct, mid = (324, 40) if what == "Ct324" else (320, 41)
    pooled, gate = (torch.full((2, 2, 2, Ct), PREFILL, device=dev) for _ in range(2))
    w, t = torch.ones(Ct * 44, device=dev), torch.ones(3 * 328, device=dev)
    rc = L.lhn_ccw_gate_fwd(_lib.ptr(pooled), 8, Ct, mid, _lib.ptr(w), _lib.ptr(t), 44, _lib.ptr(w), _lib.ptr(t), 328, _lib.ptr(gate), _lib.stream())
    torch.cuda.synchronize()
    assert rc == 1 and b"unsupported shape" in L.lhn_last_error()
    assert bool((gate == PREFILL).all())
    # the largest accepted combination, whatever the registered depths use: Ct = 320 with mid = 40, not rounded to anything
    rc = L.lhn_ccw_gate_fwd(_lib.ptr(pooled), 8, 320, 40, _lib.ptr(w), _lib.ptr(t), 44, _lib.ptr(w), _lib.ptr(t), 328, _lib.ptr(gate), _lib.stream())
    torch.cuda.synchronize()
    assert rc == 0
    if what == "Ct324":
        flat = gate.reshape(-1)                      # 8 pixels x 320 channels, written densely
        assert bool((flat[8 * 320:] == PREFILL).all()) and bool((flat[:8 * 320] != PREFILL).all())
