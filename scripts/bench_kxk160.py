"""Kernel times of the width-160 shapes next to the widths a user could pad to: `python scripts/bench_kxk160.py [H ...]` (default 64).
Dense 3x3 C -> C at batch 64 on H x H maps for C = 40, 64, 128, 160, 256 (lhn_conv_kxk_fwd / lhn_conv_kxk_bwd as
scripts/bench_kernels.py times them: bwd = dz := dy + dgrad + wgrad in one call, wgrad+dy = the same call with dx = NULL, dgrad = the
difference of the two medians), and the stem's 3 -> 40 next to 3 -> 64 on 256 x 256 images (lhn_conv_stem_fwd with statistics,
lhn_conv_stem_bwd).  Events around 20 calls after 3, five repeats: median (min..max) us.  TFLOP/s counts the useful
2 N H W C^2 9 per pass.  Each line names what the library launches (lhn_conv_kxk_route)."""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from litehandnet_amd import _lib
from litehandnet_amd._lib import View, GradView
L = _lib.lib()
dev = torch.device("cuda:0")
st = _lib.stream()


def view(t, coff=0, Cc=None, table=None):
    N, H, W, Cs = t.shape
    v = View(); v.data = t.data_ptr(); v.table = table.data_ptr() if table is not None else None
    v.gate = None
    v.N, v.H, v.W, v.cstride, v.coff, v.C = N, H, W, Cs, coff, Cc or Cs
    return v


def timeit(fn, reps=20):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3   # us


def spread(fn, n=5):
    v = sorted(timeit(fn) for _ in range(n))
    return v[n // 2], v[0], v[-1]


def table(Cs):
    t = torch.empty(3, Cs, device=dev); t[0] = 1.3; t[1] = 0.1; t[2] = 0.0
    return t


def route(bwd, N, H, Cc, feat):
    r = L.lhn_conv_kxk_route(bwd, N, H, H, Cc, Cc, 1, 16, feat, 0, -1)
    return r.decode() if r else "refused"


N = 64
print("kxk, shape, median us (min..max), TFLOP/s, launches")
for H in [int(a) for a in sys.argv[1:]] or [64]:
    for Cc in (40, 64, 128, 160, 256):
        x = torch.randn(N, H, H, Cc, device=dev); y = torch.empty(N, H, H, Cc, device=dev)
        w = torch.randn(Cc, Cc, 3, 3, device=dev) * (9 * Cc) ** -0.5
        stats = torch.zeros(32 * 2 * Cc, dtype=torch.float64, device=dev); tb = table(Cc)
        scr = torch.empty(9 * Cc * Cc, device=dev)
        vx, vy = view(x, table=tb), view(y, table=tb)
        fl = 2.0 * N * H * H * Cc * Cc * 9
        dz = torch.randn_like(y); coef = torch.randn(3, Cc, device=dev)
        g = GradView(); g.dz = dz.data_ptr(); g.dpool = None; g.coef = coef.data_ptr()
        dx = torch.empty_like(x); dw = torch.zeros(16, w.numel(), device=dev)
        fwd = lambda: _lib.check(L.lhn_conv_kxk_fwd(C.byref(vx), _lib.ptr(w), C.byref(vy), _lib.ptr(stats), 1, None, _lib.ptr(scr), st))
        bwd = lambda: _lib.check(L.lhn_conv_kxk_bwd(C.byref(vx), _lib.ptr(w), C.byref(vy), C.byref(g), _lib.ptr(dx), 0, _lib.ptr(dw), 1, 16, C.c_int64(w.numel()), _lib.ptr(scr), st))
        wgr = lambda: _lib.check(L.lhn_conv_kxk_bwd(C.byref(vx), _lib.ptr(w), C.byref(vy), C.byref(g), None, 0, _lib.ptr(dw), 1, 16, C.c_int64(w.numel()), _lib.ptr(scr), st))
        res = {}
        for name, fn, k, r in (("kxk_fwd", fwd, 1, route(0, N, H, Cc, 4)), ("kxk_bwd", bwd, 2, route(1, N, H, Cc, 5)), ("kxk_wgrad+dy", wgr, 1, route(1, N, H, Cc, 4))):
            res[name] = spread(fn)
            m, lo, hi = res[name]
            print(f"{name}, {N}x{H}x{H} {Cc}->{Cc}, {m:.1f} ({lo:.1f}..{hi:.1f}), {k * fl / m / 1e6:.1f}, {r}", flush=True)
        d = res["kxk_bwd"][0] - res["kxk_wgrad+dy"][0]
        print(f"kxk_dgrad (bwd - wgrad+dy), {N}x{H}x{H} {Cc}->{Cc}, {d:.1f}, {fl / d / 1e6:.1f}", flush=True)

print("stem 3x3 stride 2, shape, median us (min..max)")
for Co in (40, 64):
    Hi = 256
    img = torch.randn(N, 3, Hi, Hi, device=dev); y = torch.empty(N, Hi // 2, Hi // 2, Co, device=dev)
    w = torch.randn(Co, 3, 3, 3, device=dev) * 27 ** -0.5
    stats = torch.zeros(32 * 2 * Co + 64, dtype=torch.float64, device=dev); tb = table(Co)
    vy = view(y, table=tb)
    dz = torch.randn_like(y); coef = torch.randn(3, Co, device=dev)
    g = GradView(); g.dz = dz.data_ptr(); g.dpool = None; g.coef = coef.data_ptr()
    dw = torch.zeros(16, w.numel(), device=dev)
    fwd = lambda: _lib.check(L.lhn_conv_stem_fwd(_lib.ptr(img), _lib.ptr(w), C.byref(vy), _lib.ptr(stats), Hi, Hi, 3, 2, 1, None, st))
    bwd = lambda: _lib.check(L.lhn_conv_stem_bwd(_lib.ptr(img), C.byref(vy), C.byref(g), _lib.ptr(dw), Hi, Hi, 3, 2, 1, 16, C.c_int64(w.numel()), st))
    for name, fn in (("stem_fwd", fwd), ("stem_bwd", bwd)):
        m, lo, hi = spread(fn)
        print(f"{name}, {N}x3x{Hi}x{Hi} -> {Co}, {m:.1f} ({lo:.1f}..{hi:.1f})", flush=True)
