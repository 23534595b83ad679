"""Cases of the split-bf16 dense 3x3 convolution (lhn_conv_kxk_fwd_bf16x3, csrc/k_conv_kxk_bf16.hip) run through the C ABI, with
two torch references on the CPU.  v = value(x) in float32 as pw_cases._value forms it, hi(t) = bf16(t), lo(t) = bf16(t - hi(t)),
both round-to-nearest-even (torch's .to(torch.bfloat16)).
    S  what the kernel is meant to compute: conv64(hi v, hi w) + conv64(hi v, lo w) + conv64(lo v, hi w) in float64 (the first two
       as ONE convolution with hi w + lo w, which float64 holds exactly); S32 = the same three convolutions in float32
    T  the true convolution conv64(v, w);  A = conv64(|v|, |w|), the scale of the rigorous bound |S - T| <= BOUND * A
Imported by tests/test_kxk_bf16x3_gpu.py; run as a script (a child process with its own environment, e.g. LHN_DETERMINISTIC=1) it
writes the kernel outputs of the named cases to an .npz file:
    python tests/kxk_bf16x3_cases.py OUT.npz REPEATS NAME ...
    python tests/kxk_bf16x3_cases.py --check-reference        (CPU only: S stays inside BOUND * A in every case)"""
import ctypes as C
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pw_cases import PREFILL, _lib, _outside, _rand, _value, _view  # noqa: E402

PAIRS = [(ci, co) for ci in (32, 64, 128) for co in (32, 64, 128)]
SLACK = 64                      # bytes behind the split-weight scratch: must keep their fill
FILL_BYTE = 0x5A
BOUND = 3.1 * 2.0 ** -16        # |hi a * lo b| <= 2^-17 |ab| twice over, |lo a * lo b| and the second roundings below 2^-24 |ab|: per product
FLOOR = 2e-5                    # the project's kernel-level floor, relative to the largest magnitude of the reference


def _case(cin, cout, nhw, flags="", **kw):
    return dict(cin=cin, cout=cout, nhw=nhw, flags=flags.split(), **kw)


# flags: xtab: pending transform on x whose scales are negative for every third channel;  xgate;  xview: x is channels [64, 64 + Cin)
# of a wider buffer;  yview: y is channels [32, 32 + Cout) of a wider buffer;  spread: the scale of input channel c is 2^k(c), k in
# [-20, 20], and the weights of that channel carry 2^-k(c);  ints: v and w are integers in [-4, 4] (no table)
CASES = {}
for _ci, _co in PAIRS:
    CASES[f"pair_{_ci}_{_co}"] = _case(_ci, _co, (3, 9, 13), "xtab")                # 2 x 1 tiles of 8 x 16 per image, both cut by the map
CASES["one_px_64_64"] = _case(64, 64, (1, 1, 1), "xtab")                            # a map smaller than the halo
CASES["one_row_32_64"] = _case(32, 64, (1, 1, 7), "xtab")
CASES["one_col_128_32"] = _case(128, 32, (1, 7, 1), "xtab")
CASES["tiny_128_128"] = _case(128, 128, (2, 3, 3), "xtab")
CASES["tiny_64_64"] = _case(64, 64, (1, 5, 7))
CASES["tiny_32_128"] = _case(32, 128, (1, 5, 7))
CASES["below_64_128"] = _case(64, 128, (1, 15, 31), "xtab")                         # one below multiples of 8 / 16 / 32
CASES["above_128_64"] = _case(128, 64, (1, 17, 33), "xtab")                         # one above
CASES["view_64_64"] = _case(64, 64, (2, 12, 20), "xtab xgate xview yview")
CASES["view_128_32"] = _case(128, 32, (2, 12, 20), "xtab xgate xview yview")
CASES["big_128_128"] = _case(128, 128, (2, 129, 131), "xtab")                       # 2 x 17 x 9 = 306 tiles: more than resident workgroups
CASES["spread_64_64"] = _case(64, 64, (2, 9, 19), "spread")
for _ci, _co in ((128, 128), (32, 64), (64, 32)):
    CASES[f"ints_{_ci}_{_co}"] = _case(_ci, _co, (2, 9, 19), "ints")                # exact: see reference()

# calls the library must refuse (invalid-argument status, a reason, nothing written to y or to the scratch)
REFUSE = {
    "r_stride2": _case(64, 64, (2, 8, 8), "xtab half", refuse="stride 1 only"),                     # y is the stride-2 map
    "r_64_96": _case(64, 96, (2, 8, 8), "xtab", refuse="built for 32 / 64 / 128 channels"),
    "r_48_64": _case(48, 64, (2, 8, 8), "xtab", refuse="built for 32 / 64 / 128 channels"),
    "r_256_128": _case(256, 128, (2, 8, 8), "xtab", refuse="built for 32 / 64 / 128 channels"),
    "r_noscratch": _case(64, 64, (2, 8, 8), "xtab noscratch", refuse="scratch"),
    "r_overlap": _case(64, 64, (2, 8, 8), "xtab overlap", refuse="y overlaps x"),                   # y = channels [32, 96) of x's buffer
}
_ALL = dict(CASES, **REFUSE)


def geometry(name):
    """Buffer widths and channel offsets of a case: (xcs, xcoff, ycs, ycoff)."""
    c = _ALL[name]
    f = c["flags"]
    xcs, xcoff = (c["cin"] + 64, 64) if "xview" in f else (c["cin"], 0)
    ycs, ycoff = (c["cout"] + 32, 32) if "yview" in f else (c["cout"], 0)
    if "overlap" in f:
        xcs, xcoff, ycs, ycoff = 128, 0, 128, 32
    return xcs, xcoff, ycs, ycoff


def inputs(name, seed=7):
    c = _ALL[name]
    f, (n, h, w), cin, cout = c["flags"], c["nhw"], c["cin"], c["cout"]
    xcs, xcoff, _, _ = geometry(name)
    g = {"seed": seed}
    if "ints" in f:
        rng = np.random.Generator(np.random.PCG64(seed))
        g["x"] = torch.from_numpy(rng.integers(-4, 5, (n, h, w, xcs)).astype(np.float32))
        g["w"] = torch.from_numpy(rng.integers(-4, 5, (cout, cin, 3, 3)).astype(np.float32))
        return g
    g["x"] = _rand((n, h, w, xcs), seed)
    g["w"] = _rand((cout, cin, 3, 3), seed + 3, (9 * cin) ** -0.5)
    if "xtab" in f:
        sc = 1 + 0.3 * _rand((xcs,), seed + 4)
        sc[::3] = -sc[::3].abs()
        g["xtab"] = torch.stack([sc, 0.2 * _rand((xcs,), seed + 5), torch.full((xcs,), 0.1)]).contiguous()
    if "spread" in f:
        k = torch.from_numpy(np.random.Generator(np.random.PCG64(seed + 6)).integers(-20, 21, (xcs,)).astype(np.float32))
        g["xtab"] = torch.stack([torch.exp2(k), torch.zeros(xcs), torch.full((xcs,), 0.1)]).contiguous()
        g["w"] = (g["w"] * torch.exp2(-k[xcoff:xcoff + cin])[None, :, None, None]).contiguous()
    if "xgate" in f:
        g["xgate"] = torch.sigmoid(_rand((n, xcs), seed + 11))
    return g


def hi_lo(t):
    """The two bf16 parts of a float32 tensor, as float32 tensors."""
    hi = t.to(torch.bfloat16).float()
    return hi, (t - hi).to(torch.bfloat16).float()


def split_image(w):
    """What k_w_split_tapmajor leaves in the scratch: int16 [2][9][Cout][Cin], the hi image, then the lo image."""
    hi, lo = hi_lo(w)
    tm = lambda t: t.to(torch.bfloat16).view(torch.int16).reshape(w.shape[0], w.shape[1], 9).permute(2, 0, 1)  # noqa: E731
    return torch.stack([tm(hi), tm(lo)]).contiguous()


def value32(name, g):
    c = _ALL[name]
    xcs, xcoff, _, _ = geometry(name)
    sl = slice(xcoff, xcoff + c["cin"])
    cut = lambda t: (t[..., sl] if t is not None else None)  # noqa: E731
    return _value(g["x"][..., sl], cut(g.get("xtab")), cut(g.get("xgate")), torch.float32)


def _conv(v, w):
    return F.conv2d(v.permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1)


def reference(name, g=None):
    """dict(S, S32, T, A) as float64 numpy arrays [N, H, W, Cout].  `ints` cases: both lo parts are zero and every partial sum is an
    integer below 2^24 (9 * 128 * 16 = 18,432 at most), so S == T and the kernel must return exactly these bits."""
    g = g or inputs(name)
    v = value32(name, g)
    vh, vl = hi_lo(v)
    wh, wl = hi_lo(g["w"])
    d = torch.float64
    S = _conv(vh.to(d), wh.to(d) + wl.to(d)) + _conv(vl.to(d), wh.to(d))
    S32 = (_conv(vl, wh) + _conv(vh, wl)) + _conv(vh, wh)
    T = _conv(v.to(d), g["w"].to(d))
    A = _conv(v.to(d).abs(), g["w"].to(d).abs())
    return {k: t.double().numpy() for k, t in (("S", S), ("S32", S32), ("T", T), ("A", A))}


def bars(r):
    """(e32, bar_S): the float32 evaluation's error and the kernel bar against S, both relative to max |S|."""
    peak = max(float(np.abs(r["S"]).max()), 1e-30)
    e32 = float(np.abs(r["S32"] - r["S"]).max()) / peak
    return e32, max(FLOOR, 3 * e32)


# ---------------------------------------------------------------- kernel
def run(name, dev, g=None, relay=1, scratch=None, expect_fail=False):
    """One call of lhn_conv_kxk_fwd_bf16x3.  Returns y (the view's channels) and `*_ok` flags: every float outside y's channels keeps
    its prefill bit for bit, no element of y does (NaN prefill: y is fully overwritten), the scratch holds torch's split image and
    its slack.  relay=0 re-uses `scratch` (the tensor an earlier call returned under "scratch")."""
    c = _ALL[name]
    f, (n, h, w), cin, cout = c["flags"], c["nhw"], c["cin"], c["cout"]
    xcs, xcoff, ycs, ycoff = geometry(name)
    g = g or inputs(name)
    d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in g.items()}
    L, st = _lib.lib(), _lib.stream()
    vx = _view(d["x"], xcoff, cin, d.get("xtab"), d.get("xgate"))
    ho, wo = ((h + 1) // 2, (w + 1) // 2) if "half" in f else (h, w)
    nbytes = 9 * cout * cin * 4
    if "overlap" in f:
        y = d["x"]
        before = y.clone()
    else:
        y = torch.full((n, ho, wo, ycs), PREFILL, device=dev)
        y[..., ycoff:ycoff + cout] = float("nan")
        before = y.clone()
    vy = _view(y, ycoff, cout)
    scr = scratch if scratch is not None else torch.full((nbytes + SLACK,), FILL_BYTE, dtype=torch.uint8, device=dev)
    scr_before = scr.clone()
    rc = L.lhn_conv_kxk_fwd_bf16x3(C.byref(vx), _lib.ptr(d["w"]), C.byref(vy), None if "noscratch" in f else _lib.ptr(scr), relay, st)
    torch.cuda.synchronize()
    if expect_fail:
        same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))  # noqa: E731
        return rc, {"y": same(y, before), "scratch": torch.equal(scr, scr_before)}
    _lib.check(rc, f"kxk bf16x3 {name}")
    yy = y[..., ycoff:ycoff + cout]
    want = split_image(d["w"])
    return {"y": yy.cpu().numpy(), "scratch": scr,
            "y_outside_ok": np.array(bool((_outside(y, ycoff, cout) == PREFILL).all())),
            "y_written_ok": np.array(not bool(torch.isnan(yy).any())),
            "scratch_ok": np.array(torch.equal(scr[:nbytes].view(torch.int16).view(2, 9, cout, cin), want) and
                                   bool((scr[nbytes:] == FILL_BYTE).all()))}


def _check_reference():
    import time
    t0, worst32, worst_ratio = time.time(), 0.0, 0.0
    for nm in CASES:
        g = inputs(nm)
        r = reference(nm, g)
        assert all(np.isfinite(a).all() for a in r.values()), nm
        if "ints" in CASES[nm]["flags"]:
            assert np.array_equal(r["S"], r["T"]) and np.array_equal(r["S32"], r["T"]) and np.abs(r["T"]).max() < 2 ** 24, nm
            continue
        ratio = float((np.abs(r["S"] - r["T"]) / np.maximum(r["A"], 1e-300)).max())
        assert ratio <= BOUND, (nm, ratio, BOUND)
        worst_ratio = max(worst_ratio, ratio * 2.0 ** 16)
        worst32 = max(worst32, bars(r)[0])
    print(f"{len(CASES)} cases, S within {worst_ratio:.3f} * 2^-16 * conv(|v|, |w|) of the true convolution (bound 3.1), "
          f"worst float32 error {worst32:.2e}, {time.time() - t0:.1f} s")


if __name__ == "__main__":
    if sys.argv[1] == "--check-reference":
        _check_reference()
        sys.exit(0)
    dst, reps, names = sys.argv[1], int(sys.argv[2]), sys.argv[3:]
    dev = torch.device("cuda:0")
    res = {}
    for nm in names:
        g = inputs(nm)
        for r in range(reps):
            for k, v in run(nm, dev, g).items():
                if k != "scratch":
                    res[f"{nm}/{r}/{k}"] = v
    np.savez(dst, **res)
