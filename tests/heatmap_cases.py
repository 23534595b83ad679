"""Edge cases of the heat-map, loss and input-pipeline kernels (csrc/k_heatmap.hip): target encoding, arg-max / decode / refine /
back-transform, peak NMS, top-k candidates, PCK, the balanced-MSE and SimDR losses, DARK decode, affine warp, flip and HSV jitter,
run through the C ABI (the losses through litehandnet_amd.loss), with the numpy / torch oracle as reference.  Imported by
tests/test_heatmap_edges_gpu.py; run as a script:
    python tests/heatmap_cases.py OUT.npz REPEATS GROUP:NAME ...   (a child process with its own environment, e.g. LHN_DETERMINISTIC=1)
    python tests/heatmap_cases.py --check-reference                (CPU only: every case's inputs, references and input conditions)
    python tests/heatmap_cases.py --instances                      (the table of profiles/heatmap_instances.md)

Every output buffer of a C-ABI call sits in front of PAD prefilled elements; the `*_ok` flags say they kept their bits.  Each case
row names, in `why`, the path it reaches and the mistake it would catch."""
import ctypes as C
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pw_cases import PREFILL, _lib, rel_err  # noqa: E402,F401
from oracle import heatmap_np as onp  # noqa: E402
from oracle import torch_ref  # noqa: E402

PAD = 64
F32 = np.float32
TINY = float(np.finfo(np.float32).tiny)          # smallest normal float32: a positive value below it is a denormal
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
# warp: a pixel may differ by one uint8 level only where the float64 value before rounding lies within WARP_MARGIN levels of a .5
# tie.  Derived: 3 x the largest change of that value between the float64 oracle and a float32 numpy restatement of the kernel's
# coordinate arithmetic over every warp case (--check-reference measures 1.33e-3 levels and asserts 3 x measured <= WARP_MARGIN).
WARP_MARGIN = 4.0e-3
WARP_CAP = 0.05                                  # share of pixels that may be so excepted (tests/test_heatmap_gpu.py's cap)


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _step(v, up):
    return np.nextafter(F32(v), F32(np.inf if up else -np.inf))


# ---------------------------------------------------------------- case tables
ENC_MAPS = {     # name: (W, H, image w, image h); the stride is 4 on both axes everywhere, so joint / stride is exact
    "16x16": dict(W=16, H=16, iw=64, ih=64, why="H*W = 256: three quarters of the 256-thread block is idle (a thread that writes without a bound)"),
    "10x6": dict(W=10, H=6, iw=40, ih=24, why="W % 4 != 0: the float4 groups of the unbiased branch straddle rows (x = p % W taken per group, not per element)"),
    "12x40": dict(W=12, H=40, iw=48, ih=160, why="tall map, H > W: x and y bounds swapped"),
    "48x44": dict(W=48, H=44, iw=192, ih=176, why="2112 elements: two full passes of the strided loop and a partial third"),
}
ENC_SIGMAS = {   # r = 3 * sigma
    "s1": dict(sigma=1, why="float32 denormals in the unbiased map (exp(-d^2/2) for d in [13.2, 14.4]): a flushed conversion fails the 1-ulp bar"),
    "s2": dict(sigma=2, why="the deployed sigma"),
    "s3": dict(sigma=3, why="patch of 19 wider than the 10x6 / 16x16 maps: every pixel inside the patch bounds"),
    "s1.5": dict(sigma=1.5, why="3 * sigma = 4.5 is no integer: patch centre size // 2 = floor(r + 0.5) = 5, not (2 * (int)r + 1) / 2 = 4"),
}
ENC_SETS = {
    "place": "corners, far outside on each side, negative coordinates in (-stride, 0) (int() truncates toward zero), a joint outside the map "
             "whose Gaussian still reaches it, visibility 0 and 0.5 (weight stays 0.5, map zero)",
    "thr_unbiased": "the four weight-zeroing thresholds of the unbiased rule in float64, exactly on and one float32 step on either side (>= against >)",
    "thr_biased": "the four thresholds of the biased / UDP rule after int(): joint / stride + 0.5 exactly an integer and one float32 step on either side",
}
ENC = {f"{m}_{s}_{k}": dict(ENC_MAPS[m], sigma=ENC_SIGMAS[s]["sigma"], set=k, n=2, k=7, why=f"{ENC_SETS[k]}; {ENC_MAPS[m]['why']}; {ENC_SIGMAS[s]['why']}")
       for m in ENC_MAPS for s in ENC_SIGMAS for k in ENC_SETS}

AMAX = {     # 12 maps each (N = 2, K = 6), one property per map: _amax_maps
    "2x2": dict(W=2, H=2, kind="props", why="one float4: 255 threads idle, every tie inside thread 0's quad"),
    "10x6": dict(W=10, H=6, kind="props", why="15 lanes of wave 0: ties across lanes (the wave reduction takes the lower index, not the lower lane's partner)"),
    "16x16": dict(W=16, H=16, kind="props", why="exactly wave 0"),
    "36x32": dict(W=36, H=32, kind="props", why="1152 elements: ties across waves (5 / 700: LDS fold) and passes (3 / 1030: a later pass must not replace an equal earlier value)"),
    "1x80": dict(W=80, H=1, kind="props", why="H = 1 as keypoints_from_simdr calls it: y = idx / W = 0, no refine"),
    "peaks_10x6": dict(W=10, H=6, kind="peaks", why="post 1 / refine mode 0 on a non-square map: px in {0, 1, 2, W-2, W-1} x py likewise (guard 1 < p < size - 1 per axis, W and H swapped), "
                                                     "equal neighbours (sign 0), NaN neighbour (NaN shift)"),
    "peaks_36x32": dict(W=36, H=32, kind="peaks", why="as peaks_10x6 with the peak of the later maps in the second pass"),
}
OFF = {      # lhn_heatmap_refine mode 1
    "10x6": dict(W=10, H=6, why="border peaks: clamped neighbours per axis; strict > on equal neighbours; (-1, -1) rows from map 1 on load nothing and give -0.75"),
    "16x16": dict(W=16, H=16, why="as 10x6, square"),
}
NMS = {f"{m}_k{k}": dict(W=w, H=h, kernel=k, why=why + f"; kernel {k}" + ("" if k > 1 else ": every element is its own maximum"))
       for m, w, h, why in (("4x6", 4, 6, "kernel 11 wider than both sides: window clipped on every side, -inf padding"),
                            ("10x6", 10, 6, "plateaus (equal neighbours both survive), all-negative maps (suppressed values become -0.0), -0.0 inputs"),
                            ("36x32", 36, 32, "1152 elements: the second pass reads rows the first pass's threads wrote to scratch")) for k in (1, 3, 5, 11)}
TOPK = {
    "4x6_all_ties": dict(W=4, H=6, k=24, sizes=True, image=256.0, why="k = every element, values from four levels: equal values in index order; sizes below 0 and above 0.99 clipped"),
    "4x6_no_sizes": dict(W=4, H=6, k=5, sizes=False, image=256.0, why="sizes = NULL: width / height 0"),
    "128x128_k3": dict(W=128, H=128, k=3, sizes=True, image=256.0, why="the largest accepted map: 64 KiB of LDS, 16 passes per arg-max round"),
}
PCK = {
    "k300": dict(n=6, k=300, thr=0.5, why="K = 300: second pass of the k loop; zero normaliser drops a sample, negative one takes 1e6, a joint without a valid sample "
                                          "gives -1 and leaves the mean, a distance equal to the threshold is no hit (strict <)"),
    "all_masked": dict(n=3, k=5, thr=0.5, masked=True, why="every mask zero: accuracies -1, average 0, count 0 (division by a zero count)"),
}
LOSS_SHAPES = {"1x4": (1, 1, 2, 2), "3x12": (1, 3, 3, 4), "5x60": (1, 5, 6, 10), "14x256": (2, 7, 16, 16)}
LOSS_KINDS = {"half": "targets exactly 0.5 (negative) and nextafter(0.5, 1) (positive): > against >=",
              "nopos": "no positive at all: n_pos + 1 = 1 in the positive factor", "allpos": "all positive: n_neg + 1 = 1 in the negative factor"}
LOSS = {f"{s}_{k}": dict(shape=LOSS_SHAPES[s], kind=k, why=f"{LOSS_KINDS[k]}; weights 2 / 0.5 / 0, loss_weight 0.1, upstream gradient 3, balance on and off")
        for s in LOSS_SHAPES for k in LOSS_KINDS}
LOSS["stacked5d"] = dict(shape=(2, 2, 3, 4, 6), kind="half", why="5-D stacked form [N, S, K, H, W] with per-stack targets and weights")
LOSS["det_168x256"] = dict(shape=(8, 21, 16, 16), kind="half", why="43008 elements against 16 workgroups x 1024 when 2 CUs are reported: the grid-stride loop iterates")
SIMDR_ENC = {
    "k2_s1_vs1": dict(k=2, sigma=1, vs=1, why="vectors of 80 / 48 (< 256: idle threads), visibility stride 1"),
    "k3_s2_vs3": dict(k=3, sigma=2, vs=3, why="vectors of 120 / 72, visibility stride 3 (column 0 read)"),
    "k2_s2_vs3": dict(k=2, sigma=2, vs=3, why="as above at k = 2"),
    "k3_s1_vs1": dict(k=3, sigma=1, vs=1, why="as above at k = 3"),
}
SIMDR_LOSS = {"n3k5": dict(n=3, k=5, wd=80, hd=48, why="differences below 1, exactly +-1 and above 1 on both axes: both branches of smooth_l1 and of its derivative, "
                                                         "|d| < 1 strict; non-binary weights; upstream gradient 2.5")}
DARK = {f"{m}_k{k}": dict(W=w, H=h, kernel=k, why=why + f"; blur kernel {k}")
        for m, w, h, ks, why in (("16x16", 16, 16, (3, 11, 31), "peaks on both sides of the Taylor guard 1 < p < size - 2; kernel 31 wider than the map"),
                                 ("20x12", 20, 12, (3, 11), "non-square: guard per axis"),
                                 ("128x128", 128, 128, (11, 31), "the LDS cap: 2 x 64 KiB")) for k in ks}
DARKU = dict({f"{m}_k{k}": dict(W=w, H=h, kernel=k, why=why + f"; blur kernel {k}")
              for m, w, h, ks, why in (("16x16", 16, 16, (3, 11, 31), "corner and border peaks: clamped (edge-replicated) differences; reflect-101 blur with 15 taps outside"),
                                       ("20x12", 20, 12, (3, 11), "non-square: clamps per axis"),
                                       ("128x128", 128, 128, (11,), "the LDS cap"))
              for k in ks}, **{"2x2_k3": dict(W=2, H=2, kernel=3, why="the smallest map: every neighbour clamped")})
WARP = {     # N = 4: rotation 0 | 90, centre on the image corner | -180, crop wholly outside | 33.3
    "plain_40x24": dict(Wo=40, Ho=24, udp=False, flip=None, vs=1, why="non-square source and output, scale_x != scale_y, every pixel of a crop outside the image is (0 - mean) / std"),
    "flip_40x24": dict(Wo=40, Ho=24, udp=False, flip=(1, 0, 1, 1), vs=3, why="flagged sources read mirrored; invisible joints untouched; visibility stride 3"),
    "udp_40x24": dict(Wo=40, Ho=24, udp=True, flip=None, vs=3, why="UDP matrix with scale_x != scale_y; invisible joints mapped too"),
    "udp_flip_40x24": dict(Wo=40, Ho=24, udp=True, flip=(0, 1, 1, 0), vs=1, why="UDP and mirrored sources"),
    "plain_128x132": dict(Wo=128, Ho=132, udp=False, flip=None, vs=1, why="16896 pixels: second pass of the grid capped at 64 blocks"),
    "udp_128x132": dict(Wo=128, Ho=132, udp=True, flip=(1, 0, 0, 1), vs=3, why="second pass of the capped grid, UDP form"),
}
FLIP = {
    "k64_overlap": dict(n=3, k=64, vs=3, pairs=[(1, 2), (2, 3), (10, 63), (64, 5), (-1, 7)], flags=(1, 0, 1),
                        why="K = 64 (the limit); overlapping pairs (1,2),(2,3): later pairs win; pair indices out of range ignored"),
    "k1_nopairs": dict(n=2, k=1, vs=1, pairs=[], flags=(1, 1), why="K = 1, npairs = 0 with a NULL pair table; all samples flagged"),
    "k8_vs2": dict(n=3, k=8, vs=2, pairs=[(0, 7), (3, 4)], flags=(0, 1, 1), why="visibility stride 2: the third joint column takes the last visibility column"),
    "none_flagged": dict(n=3, k=8, vs=3, pairs=[(0, 7)], flags=(0, 0, 0), why="no sample flagged: nothing written"),
}
HSV = {"3x60x52": dict(n=3, h=60, w=52, why="9360 pixels x 3 images against 32 x 256 threads when 2 CUs are reported: the second pass crosses an image boundary "
                                             "(gain row taken per pixel, not per block)")}
GROUPS = {"enc": ENC, "amax": AMAX, "off": OFF, "nms": NMS, "topk": TOPK, "pck": PCK, "loss": LOSS, "simdr_enc": SIMDR_ENC, "simdr_loss": SIMDR_LOSS,
          "dark": DARK, "darku": DARKU, "warp": WARP, "flip": FLIP, "hsv": HSV}
DET = ["hsv:3x60x52", "loss:det_168x256"]        # the child process of LHN_DETERMINISTIC=1
KERNELS = {"enc": "k_encode", "amax": "k_decode, k_refine, k_transform", "off": "k_refine (mode 1)", "nms": "k_nms", "topk": "k_topk_candidates", "pck": "k_pck",
           "loss": "k_loss_fwd, k_loss_final, k_loss_bwd", "simdr_enc": "k_simdr_encode", "simdr_loss": "k_simdr_loss_sums, k_simdr_loss_final, k_simdr_loss_bwd",
           "dark": "k_dark", "darku": "k_dark_udp", "warp": "k_affine_warp_norm, k_affine_joints", "flip": "k_flip_joints", "hsv": "k_hsv_jitter"}


# ---------------------------------------------------------------- inputs
def _enc_joints(c):
    W, H, iw, ih, r = c["W"], c["H"], c["iw"], c["ih"], 3 * c["sigma"]
    sx, sy = iw / W, ih / H
    j = np.zeros((14, 3), F32)
    v = np.ones((14, 3), F32)
    inx, iny = F32(sx * 1.0), F32(sy * 1.0)                 # the other coordinate of a threshold joint: heat-map pixel 1
    if c["set"] == "place":
        j[:4, :2] = [(0, 0), (iw - 1, 0), (0, ih - 1), (iw - 1, ih - 1)]
        j[4:8, :2] = [(-1000, ih / 2), (iw + 1000, ih / 2), (iw / 2, -1000), (iw / 2, ih + 1000)]
        j[8:11, :2] = [(-1.5, 5.25), (6.5, -3.9), (-0.3, -2.2)]
        j[11, :2] = (sx * (W + r - 0.25), 0)                # outside, inside the unbiased threshold: far pixels are denormal at sigma = 1
        j[12, :2], v[12] = (iw * 0.37, ih * 0.61), 0
        j[13, :2], v[13] = (iw * 0.52, ih * 0.33), 0.5
    else:
        if c["set"] == "thr_unbiased":                      # mx - r >= W | my - r >= H | mx + r + 1 < 0 | my + r + 1 < 0 in float64
            xs = [sx * (W + r), sy * (H + r), -sx * (r + 1), -sy * (r + 1)]
        else:                                               # int(mx - r) >= W, int(mx + r + 1) < 0 with mx = int(joint / stride + 0.5)
            hi = lambda size: float(np.ceil(size + r)) - 0.5                   # noqa: E731   joint / stride + 0.5 = ceil(size + r): ul = size
            lo = float(np.floor(-(r + 2))) - 0.5                                # joint / stride + 0.5 = floor(-(r + 2)): br = -1
            xs = [sx * hi(W), sy * hi(H), sx * lo, sy * lo]
        i = 0
        for t, val in enumerate(xs):
            for q in (F32(val), _step(val, True), _step(val, False)):
                j[i, :2] = (q, iny) if t % 2 == 0 else (inx, q)
                i += 1
        j[12, :2] = (sx * (W + r - 0.25), 0)                # as in "place": denormal far pixels at sigma = 1 on every map
        j[13, :2], v[13] = (iw * 0.6 + 0.3, ih * 0.2 - 0.2), 0.5
    return j.reshape(2, 7, 3), v.reshape(2, 7, 3)


def _amax_maps(W, H, rng):
    HW = W * H
    base = lambda: rng.uniform(0.1, 0.5, HW).astype(F32)   # noqa: E731

    def put(idx, val):
        m = base()
        for i, x in zip(idx, val if isinstance(val, (list, tuple)) else [val] * len(idx)):
            m[min(i, HW - 1)] = x
        return m
    return np.stack([
        put((1, 2), 0.9),                      # the maximum twice in one float4: the later element of a quad must not win
        put((2, 4 * 37 + 1), 0.9),             # twice in one wave (lanes 0 and 37): the shuffle reduction keeps the lower index
        put((5, 700), 0.9),                    # in two waves: the fold over the four wave results
        put((3, 1030), 0.9),                   # in two passes of the strided loop (thread 0 / thread 1 of pass 2)
        put((HW // 3, HW - 1), 0.9),           # second occurrence is the last element
        np.full(HW, 0.25, F32),                # all equal: index 0
        np.full(HW, -np.inf, F32),             # all -inf: index 0 although nothing beats the initial -inf; prediction -1
        -base(),                               # all negative: prediction -1 and the back-transform of -1
        put((6, 900), np.inf),                 # +inf twice
        put((2, 9), [0.9, np.nan]),            # one NaN after a larger finite value: NaN is the maximum
        put((7, 300), np.nan),                 # two NaNs: the first
        base(),                                # no tie
    ]).reshape(2, 6, H, W)


def _peak_maps(W, H, rng):
    """27 maps: 25 peaks at px, py in {0, 1, 2, size - 2, size - 1}, one with equal neighbours on both axes, one with a NaN neighbour."""
    hm = rng.uniform(0.1, 0.5, (27, H, W)).astype(F32)
    xy = [(px, py) for py in (0, 1, 2, H - 2, H - 1) for px in (0, 1, 2, W - 2, W - 1)] + [(W // 2, H // 2), (W // 2 - 1, H // 2)]
    for m, (px, py) in zip(hm, xy):
        m[py, px] = 0.9
    m = hm[25]
    px, py = xy[25]
    m[py, px - 1] = m[py, px + 1] = 0.3
    m[py - 1, px] = m[py + 1, px] = 0.2
    px, py = xy[26]
    hm[26][py, px + 1] = np.nan
    return hm.reshape(3, 9, H, W), np.array(xy, F32).reshape(3, 9, 2)


def _cs(n):
    return (np.array([[31.0, 20.5], [17.25, 44.0], [52.5, 9.75], [40.0, 40.0]], F32)[:n].copy(),
            np.array([[0.31, 0.47], [0.55, 0.29], [0.2, 0.26], [0.4, 0.3]], F32)[:n].copy())


def _blob(W, H, cx, cy, rng, amp=0.8, s=2.0):
    ys, xs = np.mgrid[0:H, 0:W]
    return (amp * np.exp(-((xs - cx) ** 2 + (ys - cy) ** 2) / (2 * s * s)) + rng.uniform(0, 0.01, (H, W))).astype(F32)


def _dark_maps(c, udp, seed):
    W, H = c["W"], c["H"]
    rng = _rng(seed)
    if W == 2:
        xy = [(0, 0), (1, 0), (0, 1), (1, 1)]
    else:
        xy = [(px, H // 2) for px in (1, 2, W - 3, W - 2)] + [(W // 2, py) for py in (1, 2, H - 3, H - 2)] + [(W // 2 - 1, H // 2 + 1)]
        if udp:
            xy += [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]
    maps = [_blob(W, H, px + 0.3, py - 0.2, rng, s=0.8 if W == 2 else 2.0) for px, py in xy]
    neg = [-_blob(W, H, W / 2, H / 2, rng) for _ in range(2 if udp else 1)]         # non-positive maps: prediction -1
    maps += neg
    n = 3 if len(maps) % 3 == 0 else (2 if len(maps) % 2 == 0 else 1)
    g = dict(hm=np.stack(maps).reshape(n, len(maps) // n, H, W), peaks=np.array(xy, F32), nneg=len(neg))
    g["center"], g["scale"] = _cs(n)
    return g


def inputs(group, name, seed=11):
    c = GROUPS[group][name]
    rng = _rng(seed + sum(map(ord, group + name)))
    g = {}
    if group == "enc":
        g["joints"], g["vis"] = _enc_joints(c)
    elif group == "amax":
        W, H = c["W"], c["H"]
        if c["kind"] == "props":
            g["hm"] = _amax_maps(W, H, rng)
            with np.errstate(invalid="ignore"):
                g["coords"] = onp.get_max_preds(g["hm"])[0]
        else:
            g["hm"], g["coords"] = _peak_maps(W, H, rng)
        g["center"], g["scale"] = _cs(g["hm"].shape[0])
        with np.errstate(invalid="ignore"):
            g["coords_t"] = onp.refine_default(g["hm"], g["coords"])
    elif group == "off":
        W, H = c["W"], c["H"]
        xy = [(px, py) for py in (0, 1, H - 2, H - 1) for px in (0, 1, W - 2, W - 1)] + [(W // 2, H // 2)] + [(-1, -1)] * 3
        hm = rng.uniform(0.1, 0.9, (20, H, W)).astype(F32)
        hm[16] = 0.4                                          # equal neighbours: strict > gives -0.25
        g["hm"], g["coords"] = hm.reshape(2, 10, H, W), np.array(xy, F32).reshape(2, 10, 2)
    elif group == "nms":
        W, H = c["W"], c["H"]
        hm = np.stack([rng.integers(0, 4, (H, W)) / 4, rng.integers(0, 3, (H, W)) / 2,                # plateaus
                       -rng.uniform(0.1, 1, (H, W)), -rng.integers(1, 4, (H, W)) / 4,                   # all negative
                       np.where(rng.random((H, W)) < 0.5, -0.0, 0.0), rng.standard_normal((H, W))]).astype(F32)
        g["hm"] = hm.reshape(2, 3, H, W)
    elif group == "topk":
        W, H = c["W"], c["H"]
        g["centre"] = (rng.integers(0, 4, (2, H, W)) / 4 if "ties" in name else rng.standard_normal((2, H, W))).astype(F32)
        if c["sizes"]:
            g["sizes"] = rng.uniform(-0.3, 1.3, (2, 2, H, W)).astype(F32)
    elif group == "pck":
        n, k = c["n"], c["k"]
        g["gt"] = rng.uniform(0, 64, (n, k, 2)).astype(F32)
        g["pred"] = (g["gt"] + rng.uniform(-1, 1, (n, k, 2)) * np.array([1, 2, 1e5, 1, 1, 1][:n] if n == 6 else [1] * n)[:, None, None]).astype(F32)
        g["mask"] = (rng.random((n, k)) < 0.8)
        g["normalize"] = np.array([[1, 1], [2, 0], [-1, 2], [2, 2], [1.5, 1.5], [0, 0]], F32)[:n].copy() if n == 6 else np.ones((n, 2), F32)
        if c.get("masked"):
            g["mask"][:] = False
        else:
            g["mask"][:, 7] = False                           # joint 7: no valid sample
            g["mask"][:, 3] = True                            # joint 3: distance exactly thr (0.5 x normaliser, 0) in every kept sample
            g["pred"][:, 3] = g["gt"][:, 3]
            g["gt"][:, 3] = np.rint(g["gt"][:, 3])
            g["pred"][:, 3, 0] = g["gt"][:, 3, 0] + 0.5 * np.abs(g["normalize"][:, 0])
            g["pred"][:, 3, 1] = g["gt"][:, 3, 1]
            g["pred"][2, 3] = g["gt"][2, 3]                   # (the 1e6 route: distance 0)
    elif group == "loss":
        shp = c["shape"]
        g["out"] = (0.5 + 0.4 * rng.standard_normal(shp)).astype(F32)
        above = np.nextafter(F32(0.5), F32(1))
        if c["kind"] == "half":
            t = rng.choice(np.array([0.0, 0.25, 0.5, above, 0.9], F32), shp)
        elif c["kind"] == "nopos":
            t = rng.choice(np.array([0.0, 0.25, 0.5], F32), shp)
        else:
            t = rng.choice(np.array([above, 0.75, 1.0], F32), shp)
        g["target"] = t.astype(F32)
        nw = int(np.prod(shp[:-2]))
        g["weight"] = np.array([2.0, 0.5, 0.0], F32)[np.arange(nw) % 3].reshape(shp[:-2] + (1,))
    elif group == "simdr_enc":
        j = np.zeros((2, 5, 3), F32)
        j[..., :2] = rng.uniform(2, 22, (2, 5, 2))
        j[0, 1, :2], j[0, 2, :2], j[1, 0, :2] = (-3.3, 26.1), (42.2, -2.4), (39.4, 23.3)          # off either end of x / y, the end value still normal
        v = np.ones((2, 5, c["vs"]), F32)
        v[0, 3], v[1, 4] = 0, 0
        if c["vs"] == 3:
            v[0, 0, 1:] = 0                                   # only column 0 decides
        g["joints"], g["vis"] = j, v
    elif group == "simdr_loss":
        n, k, wd, hd = c["n"], c["k"], c["wd"], c["hd"]
        dset = np.array([0.25, -0.5, 0.875, 1.0, -1.0, 1.5, -3.0, 0.0, -0.125, 1.0, -1.0, 2.25], F32)   # exact in float32: p - t = d in every bit
        for a, L in (("x", wd), ("y", hd)):
            t = (rng.integers(0, 9, (n, k, L)) / 8).astype(F32)
            d = dset[(np.arange(n * k * L) + (3 if a == "y" else 0)) % len(dset)].reshape(n, k, L)
            g["t" + a], g["d" + a], g["p" + a] = t, d, (t + d).astype(F32)
        g["weight"] = rng.uniform(0, 2, (n, k)).astype(F32)
    elif group in ("dark", "darku"):
        g = _dark_maps(c, group == "darku", seed + sum(map(ord, name)))
    elif group == "warp":
        Ws, Hs, K = 37, 53, 6
        g["img"] = rng.integers(0, 256, (4, Hs, Ws, 3), dtype=np.uint8)
        g["center"] = np.array([[18.3, 26.1], [0.0, 0.0], [400.0, -300.0], [20.7, 24.4]], F32)
        g["scale"] = np.array([[0.23, 0.31], [0.19, 0.27], [0.21, 0.17], [0.29, 0.22]], F32) * (1.0 if c["Wo"] == 40 else 0.93)
        g["rot"] = np.array([0.0, 90.0, -180.0, 33.3], F32)
        j = np.zeros((4, K, 3), F32)
        j[..., :2] = rng.uniform(-5, 55, (4, K, 2))
        v = np.ones((4, K, c["vs"]), F32)
        v[0, 2], v[3, 0] = 0, 0
        g["joints"], g["vis"] = j, v
    elif group == "flip":
        n, k, vs = c["n"], c["k"], c["vs"]
        j = rng.uniform(0, 50, (n, k, 3)).astype(F32)
        v = (rng.random((n, k, vs)) < 0.7).astype(F32)
        g["joints"], g["vis"], g["center"] = j, v, rng.uniform(5, 45, (n, 2)).astype(F32)
    elif group == "hsv":
        g["img"] = rng.integers(0, 256, (c["n"], c["h"], c["w"], 3), dtype=np.uint8)
        g["img"][0, :3] = rng.integers(0, 256, (3, c["w"], 1), dtype=np.uint8)      # grey rows: s = 0
        g["gains"] = np.array([[5, -30, 17], [-4, 22, -30], [0, 0, 0], [3, 30, 30]], np.int16)[:c["n"]].copy()
    return g


# ---------------------------------------------------------------- reference
def _xform(coords, center, scale, size, udp):
    with np.errstate(invalid="ignore"):
        return np.stack([onp.transform_preds(coords[i], center[i], scale[i], size, udp) for i in range(coords.shape[0])])


def _warp_pre32(img, center, scale, rot, Wo, Ho, udp):
    """The kernel's coordinate arithmetic and bilinear sum restated in float32 numpy: the value before the uint8 rounding, [Ho, Wo, 3]."""
    f = F32
    r = f(rot) * f(3.14159265358979323846) / f(180)
    cr, sr = np.cos(r, dtype=F32), np.sin(r, dtype=F32)
    if not udp:
        inv = f(scale[0]) * f(200) / f(Wo)
        a00, a01, a10, a11 = inv * cr, -inv * sr, inv * sr, inv * cr
        qx, qy, px, py = f(center[0]), f(center[1]), f(0.5) * f(Wo), f(0.5) * f(Ho)
    else:
        tw, th, iw, ih = f(scale[0]) * f(200), f(scale[1]) * f(200), f(center[0]) * f(2), f(center[1]) * f(2)
        sx, sy = (f(Wo) - f(1)) / tw, (f(Ho) - f(1)) / th
        a00, a01, a10, a11 = cr / sx, sr / sy, -sr / sx, cr / sy
        qx = qy = f(0)
        px = sx * (f(-0.5) * iw * cr + f(0.5) * ih * sr + f(0.5) * tw)
        py = sy * (f(-0.5) * iw * sr - f(0.5) * ih * cr + f(0.5) * th)
    ys, xs = np.mgrid[0:Ho, 0:Wo].astype(F32)
    dx, dy = xs - px, ys - py
    sx_, sy_ = qx + a00 * dx + a01 * dy, qy + a10 * dx + a11 * dy
    fx, fy = np.floor(sx_), np.floor(sy_)
    x0, y0, ax, ay = fx.astype(np.int64), fy.astype(np.int64), sx_ - fx, sy_ - fy
    Hs, Ws = img.shape[:2]
    out = np.zeros((Ho, Wo, 3), F32)
    for j in (0, 1):
        for i in (0, 1):
            xx, yy = x0 + i, y0 + j
            ok = (xx >= 0) & (xx < Ws) & (yy >= 0) & (yy < Hs)
            wgt = ((ax if i else f(1) - ax) * (ay if j else f(1) - ay)).astype(F32)
            out += (wgt * ok)[..., None] * img[np.clip(yy, 0, Hs - 1), np.clip(xx, 0, Ws - 1)].astype(F32)
    return out


def _simdr_crit(px, py, tx, ty, w):
    """torch_ref.SimDRLoss's criterion on the decoded vectors (torch_ref.py: per joint, SmoothL1 mean x the mean of that joint's weights)."""
    K = px.size(1)
    total = 0
    for j in range(K):
        mw = w[:, j].reshape(-1).mean()
        total = total + F.smooth_l1_loss(px[:, j], tx[:, j]) * mw + F.smooth_l1_loss(py[:, j], ty[:, j]) * mw
    return total / K


def reference(group, name, g=None, dtype=np.float64):
    """dtype: float64, or float32 to measure what the same reference loses in the kernels' precision (loss, simdr_loss, dark, darku)."""
    c = GROUPS[group][name]
    g = g or inputs(group, name)
    out = {}
    if group == "enc":
        isz, hsz = [c["iw"], c["ih"]], [c["W"], c["H"]]
        for mode in (0, 1, 2):
            fn = (lambda j, v: onp.udp_generate_target(j, v, isz, hsz, c["sigma"])) if mode == 2 else \
                 (lambda j, v: onp.msra_generate_target(j, v, isz, hsz, c["sigma"], mode == 1))           # noqa: E731
            tw = [fn(j, v) for j, v in zip(g["joints"], g["vis"])]
            out[f"t{mode}"], out[f"w{mode}"] = np.stack([a for a, _ in tw]), np.stack([b for _, b in tw])
    elif group == "amax":
        hm, W, H = g["hm"], c["W"], c["H"]
        with np.errstate(invalid="ignore"):
            out["preds"], out["maxvals"] = onp.get_max_preds(hm)
            out["index"] = hm.reshape(hm.shape[0], hm.shape[1], -1).argmax(2).astype(np.int32)
            for post, pp in ((0, None), (1, "default")):
                out[f"hm_preds{post}"], out[f"preds{post}"], out[f"maxvals{post}"] = onp.keypoints_from_heatmaps(hm, g["center"], g["scale"], pp)
            out["refined"] = onp.refine_default(hm, g["coords"])
        out["xform"] = _xform(g["coords_t"], g["center"], g["scale"], [W, H], False)
        if H > 1:
            out["xform_udp"] = _xform(g["coords_t"], g["center"], g["scale"], [W, H], True)
    elif group == "off":
        out["refined"] = onp.refine_offset_legacy(g["hm"], g["coords"])
    elif group == "nms":
        out["hm"] = onp.heatmap_nms(g["hm"], c["kernel"])
    elif group == "topk":
        out["cand"] = onp.candidate_bbox(g["centre"], g.get("sizes"), c["k"], c["image"])
    elif group == "pck":
        acc, avg, cnt = onp.keypoint_pck_accuracy(g["pred"], g["gt"], g["mask"], c["thr"], g["normalize"])
        out["acc"], out["avg"], out["cnt"] = np.asarray(acc, np.float64), np.float64(avg), np.int64(cnt)
    elif group == "loss":
        dt = torch.float64 if dtype == np.float64 else torch.float32
        for bal in (1, 0):
            o = torch.from_numpy(g["out"]).to(dt).requires_grad_()
            loss = 0.1 * torch_ref.distance_loss(o, torch.from_numpy(g["target"]).to(dt), torch.from_numpy(g["weight"]).to(dt), bool(bal))
            (3 * loss).backward()
            out[f"loss_b{bal}"], out[f"grad_b{bal}"] = loss.detach().double().numpy().reshape(1), o.grad.double().numpy()
    elif group == "simdr_enc":
        xy = [onp.generate_sa_simdr(j, v, [40, 24], c["k"], c["sigma"]) for j, v in zip(g["joints"], g["vis"])]
        out["tx"], out["ty"] = np.stack([a for a, _ in xy]), np.stack([b for _, b in xy])
    elif group == "simdr_loss":
        dt = torch.float64 if dtype == np.float64 else torch.float32
        px, py = (torch.from_numpy(g[k]).to(dt).requires_grad_() for k in ("px", "py"))
        loss = _simdr_crit(px, py, torch.from_numpy(g["tx"]).to(dt), torch.from_numpy(g["ty"]).to(dt), torch.from_numpy(g["weight"]).to(dt))
        (2.5 * loss).backward()
        out["loss"], out["dpx"], out["dpy"] = loss.detach().double().numpy().reshape(1), px.grad.double().numpy(), py.grad.double().numpy()
    elif group in ("dark", "darku"):
        fn = onp.keypoints_from_heatmaps_udp if group == "darku" else (lambda h, ce, sc, k, dtype: onp.keypoints_from_heatmaps(h, ce, sc, "unbiased", k, dtype))
        with np.errstate(invalid="ignore", divide="ignore"):
            hp, pr, mv = fn(g["hm"], g["center"], g["scale"], c["kernel"], dtype=dtype)
        out["hm_preds"], out["preds"], out["maxvals"] = hp.astype(np.float64), pr.astype(np.float64), mv
    elif group == "warp":
        Wo, Ho = c["Wo"], c["Ho"]
        res, js, pre = [], g["joints"].astype(np.float64).copy(), []
        for n in range(4):
            img = g["img"][n][:, ::-1] if c["flip"] and c["flip"][n] else g["img"][n]
            r, M, p = onp.warp_affine_normalize(np.ascontiguousarray(img), g["center"][n], g["scale"][n], g["rot"][n], [Wo, Ho], use_udp=c["udp"], return_pre=True)
            res.append(r)
            pre.append(p)
            mapped = np.concatenate([g["joints"][n, :, :2].astype(np.float64), np.ones((js.shape[1], 1))], 1) @ M.T
            keep = (g["vis"][n, :, 0] > 0) | c["udp"]
            js[n, keep, :2] = mapped[keep]
        out["out"], out["joints"], out["_pre"] = np.stack(res), js, np.stack(pre).transpose(0, 3, 1, 2)
    elif group == "flip":
        j, v, ce = g["joints"].copy(), g["vis"].copy(), g["center"].copy()
        vs, K = c["vs"], c["k"]
        pairs = [p for p in c["pairs"] if 0 <= p[0] < K and 0 <= p[1] < K]           # (the reference would index out of range)
        for n in range(c["n"]):
            if c["flags"][n]:
                v3 = g["vis"][n][:, [min(q, vs - 1) for q in range(3)]]
                _, jn, vn, cn = onp.random_flip(np.zeros((1, 50, 3), np.uint8), g["joints"][n], v3, g["center"][n], pairs)
                j[n], v[n], ce[n] = jn, vn[:, :vs], cn
        out["joints"], out["vis"], out["center"] = j, v, ce
    elif group == "hsv":
        out["img"] = np.stack([onp.hsv_jitter(im, gn) for im, gn in zip(g["img"], g["gains"])])
    return out


# ---------------------------------------------------------------- kernels
def _alloc(shape, dev, init=None, dtype=torch.float32):
    """A tensor of `shape` in front of PAD more elements, all PREFILL (or `init`): (flat buffer, view)."""
    cnt = int(np.prod(shape))
    flat = torch.full((cnt + PAD,), PREFILL, device=dev, dtype=dtype)
    if init is not None:
        flat[:cnt] = torch.as_tensor(init).to(dev).reshape(-1)
    return flat, flat[:cnt].view(tuple(shape))


def run(group, name, dev, g=None):
    """Outputs as numpy arrays plus `*_ok` flags: the PAD elements behind every output buffer kept their prefill."""
    c = GROUPS[group][name]
    g = g or inputs(group, name)
    L, st, p, fl = _lib.lib(), _lib.stream(), _lib.ptr, C.c_float
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in g.items() if isinstance(v, np.ndarray)}
    out, bufs = {}, {}

    def ob(key, shape, init=None, dtype=torch.float32):
        bufs[key] = _alloc(shape, dev, init, dtype)
        return bufs[key][1]

    def call(rc, what):
        _lib.check(rc, f"{group}:{name} {what}")

    def fin(rename=None):
        torch.cuda.synchronize()
        for k, (flat, t) in bufs.items():
            out[(rename or {}).get(k, k)] = t.cpu().numpy()
            out[k + "_pad_ok"] = np.array(bool((flat[t.numel():] == PREFILL).all()))
        bufs.clear()

    if group == "enc":
        N, K = d["joints"].shape[:2]
        for mode in (0, 1, 2):
            t, w = ob(f"t{mode}", (N, K, c["H"], c["W"])), ob(f"w{mode}", (N, K, 1))
            call(L.lhn_heatmap_encode(p(d["joints"]), p(d["vis"]), p(t), p(w), N, K, c["H"], c["W"], fl(c["iw"]), fl(c["ih"]), fl(c["sigma"]), mode, st), f"mode {mode}")
        fin()
    elif group == "amax":
        hm = d["hm"]
        N, K, H, W = hm.shape
        call(L.lhn_heatmap_argmax(p(hm), p(ob("preds", (N, K, 2))), p(ob("maxvals", (N, K, 1))), p(ob("index", (N, K), dtype=torch.int32)), N, K, H, W, st), "argmax")
        for post in (0, 1):
            call(L.lhn_heatmap_decode(p(hm), p(d["center"]), p(d["scale"]), p(ob(f"hm_preds{post}", (N, K, 2))), p(ob(f"preds{post}", (N, K, 2))),
                                      p(ob(f"maxvals{post}", (N, K, 1))), N, K, H, W, post, st), f"decode {post}")
        call(L.lhn_heatmap_refine(p(hm), p(ob("refined", (N, K, 2), d["coords"])), N, K, H, W, 0, st), "refine 0")
        call(L.lhn_transform_preds(p(d["coords_t"]), p(d["center"]), p(d["scale"]), p(ob("xform", (N, K, 2))), N, K, W, H, 0, st), "transform")
        if H > 1:
            call(L.lhn_transform_preds(p(d["coords_t"]), p(d["center"]), p(d["scale"]), p(ob("xform_udp", (N, K, 2))), N, K, W, H, 1, st), "transform udp")
        fin()
    elif group == "off":
        N, K, H, W = d["hm"].shape
        call(L.lhn_heatmap_refine(p(d["hm"]), p(ob("refined", (N, K, 2), d["coords"])), N, K, H, W, 1, st), "refine 1")
        fin()
    elif group == "nms":
        N, K, H, W = d["hm"].shape
        call(L.lhn_heatmap_nms(p(ob("hm", (N, K, H, W), d["hm"])), p(ob("scratch", (N, K, H, W))), N, K, H, W, c["kernel"], st), "nms")
        fin()
        del out["scratch"]
    elif group == "topk":
        N, H, W = d["centre"].shape
        call(L.lhn_heatmap_topk(p(d["centre"]), p(d.get("sizes")), p(ob("cand", (N, c["k"], 5))), N, H, W, c["k"], fl(c["image"]), st), "topk")
        fin()
    elif group == "pck":
        N, K = d["mask"].shape
        mask = d["mask"].to(torch.uint8).contiguous()
        call(L.lhn_pck_accuracy(p(d["pred"]), p(d["gt"]), p(mask), p(d["normalize"]), fl(c["thr"]), p(ob("acc", (K,))), p(ob("avg_cnt", (2,))),
                                N, K, st), "pck")
        fin()
        out["avg"], out["cnt"] = np.float64(out["avg_cnt"][0]), np.int64(out["avg_cnt"][1])
    elif group == "loss":
        from litehandnet_amd.loss import DistanceLoss
        for bal in (1, 0):
            o = d["out"].clone().requires_grad_()
            loss = DistanceLoss(balance=bool(bal))(o, d["target"], d["weight"], 0.1)
            (3 * loss).backward()
            out[f"loss_b{bal}"], out[f"grad_b{bal}"] = loss.detach().cpu().numpy().reshape(1), o.grad.cpu().numpy()
        out["inputs_ok"] = np.array(torch.equal(d["out"].cpu(), torch.from_numpy(g["out"])) and torch.equal(d["target"].cpu(), torch.from_numpy(g["target"])))
    elif group == "simdr_enc":
        N, K = d["joints"].shape[:2]
        Wd, Hd = 40 * c["k"], 24 * c["k"]
        call(L.lhn_simdr_encode(p(d["joints"]), p(d["vis"]), c["vs"], p(ob("tx", (N, K, Wd))), p(ob("ty", (N, K, Hd))), N, K, Wd, Hd, fl(c["k"]), fl(c["sigma"]), st), "encode")
        fin()
    elif group == "simdr_loss":
        N, K, Wd, Hd = c["n"], c["k"], c["wd"], c["hd"]
        sums = ob("sums", (3 * K,), dtype=torch.float64)
        call(L.lhn_simdr_loss_fwd(p(d["px"]), p(d["py"]), p(d["tx"]), p(d["ty"]), p(d["weight"]), p(sums), p(ob("loss", (1,))), N, K, Wd, Hd, st), "fwd")
        gout = torch.full((1,), 2.5, device=dev)
        call(L.lhn_simdr_loss_bwd(p(d["px"]), p(d["py"]), p(d["tx"]), p(d["ty"]), p(sums), p(gout), p(ob("dpx", (N, K, Wd))), p(ob("dpy", (N, K, Hd))), N, K, Wd, Hd, st), "bwd")
        fin()
        del out["sums"]
    elif group in ("dark", "darku"):
        N, K, H, W = d["hm"].shape
        fn = L.lhn_heatmap_decode_dark_udp if group == "darku" else L.lhn_heatmap_decode_dark
        call(fn(p(d["hm"]), p(d["center"]), p(d["scale"]), p(ob("hm_preds", (N, K, 2))), p(ob("preds", (N, K, 2))), p(ob("maxvals", (N, K, 1))), N, K, H, W, c["kernel"], st), "dark")
        fin()
    elif group == "warp":
        N, Hs, Ws, _ = d["img"].shape
        K = d["joints"].shape[1]
        m3, s3 = (fl * 3)(*MEAN), (fl * 3)(*STD)
        flp = torch.tensor(c["flip"], dtype=torch.uint8, device=dev) if c["flip"] else None
        call(L.lhn_affine_warp_normalize2(p(d["img"]), N, Hs, Ws, p(d["center"]), p(d["scale"]), p(d["rot"]), m3, s3, p(ob("out", (N, 3, c["Ho"], c["Wo"]))), c["Ho"], c["Wo"],
                                          p(ob("joints", (N, K, 3), d["joints"])), p(d["vis"]), c["vs"], K, int(c["udp"]), p(flp), st), "warp")
        fin()
    elif group == "flip":
        N, K, vs = c["n"], c["k"], c["vs"]
        pr = torch.tensor(c["pairs"], dtype=torch.int32, device=dev).reshape(-1, 2) if c["pairs"] else None
        flg = torch.tensor(c["flags"], dtype=torch.uint8, device=dev)
        call(L.lhn_random_flip(p(ob("joints", (N, K, 3), d["joints"])), p(ob("vis", (N, K, vs), d["vis"])), vs, p(ob("center", (N, 2), d["center"])), p(flg), p(pr), len(c["pairs"]),
                               N, K, 50, st), "flip")
        fin()
    elif group == "hsv":
        N, H, W, _ = d["img"].shape
        call(L.lhn_hsv_jitter(p(ob("img", (N, H, W, 3), d["img"], torch.uint8)), p(d["gains"]), N, H, W, st), "hsv")
        fin()
    return out


# ---------------------------------------------------------------- calls the library must refuse
def _refuse_rows():
    i64, fl = C.c_int64, C.c_float
    return {    # name: (call(L, f, d8, u8, st) -> status; f / d8 / u8: float32 / float64 / uint8 buffers), text lhn_last_error must hold)
        "encode_hw_mod4": (lambda L, f, d8, u8, st: L.lhn_heatmap_encode(f[0], f[1], f[2], f[3], 2, 3, 3, 3, fl(12), fl(12), fl(2), 1, st), "lhn_heatmap_encode: bad shape"),
        "argmax_hw_mod4": (lambda L, f, d8, u8, st: L.lhn_heatmap_argmax(f[0], f[1], f[2], f[3], 2, 3, 5, 5, st), "lhn_heatmap_argmax: bad shape"),
        "decode_hw_mod4": (lambda L, f, d8, u8, st: L.lhn_heatmap_decode(f[0], f[1], f[2], f[3], f[4], f[5], 2, 3, 3, 6, 1, st), "multiple of 4"),
        "loss_fwd_hw_mod4": (lambda L, f, d8, u8, st: L.lhn_loss_balanced_mse_fwd(f[0], f[1], f[2], d8[0], f[3], i64(6), i64(10), fl(1), 1, st), "lhn_loss_balanced_mse_fwd: bad shape"),
        "loss_bwd_hw_mod4": (lambda L, f, d8, u8, st: L.lhn_loss_balanced_mse_bwd(f[0], f[1], f[2], d8[0], f[3], f[4], i64(6), i64(10), fl(1), 1, st), "lhn_loss_balanced_mse_bwd: bad shape"),
        "dark_hw_gt_16384": (lambda L, f, d8, u8, st: L.lhn_heatmap_decode_dark(f[0], f[1], f[2], f[3], f[4], f[5], 1, 1, 132, 128, 11, st), "<= 16384"),
        "dark_udp_hw_gt_16384": (lambda L, f, d8, u8, st: L.lhn_heatmap_decode_dark_udp(f[0], f[1], f[2], f[3], f[4], f[5], 1, 1, 132, 128, 11, st), "<= 16384"),
        "topk_hw_gt_16384": (lambda L, f, d8, u8, st: L.lhn_heatmap_topk(f[0], f[1], f[2], 1, 132, 128, 3, fl(256), st), "<= 16384"),
        "dark_even_kernel": (lambda L, f, d8, u8, st: L.lhn_heatmap_decode_dark(f[0], f[1], f[2], f[3], f[4], f[5], 1, 2, 16, 16, 4, st), "kernel 4 (odd, 3..31)"),
        "dark_kernel_33": (lambda L, f, d8, u8, st: L.lhn_heatmap_decode_dark(f[0], f[1], f[2], f[3], f[4], f[5], 1, 2, 16, 16, 33, st), "kernel 33 (odd, 3..31)"),
        "dark_udp_even_kernel": (lambda L, f, d8, u8, st: L.lhn_heatmap_decode_dark_udp(f[0], f[1], f[2], f[3], f[4], f[5], 1, 2, 16, 16, 12, st), "kernel 12 (odd, 3..31)"),
        "flip_k65": (lambda L, f, d8, u8, st: L.lhn_random_flip(f[0], f[1], 3, f[2], u8[0], f[3], 1, 2, 65, 50, st), "K <= 64"),
        "pck_k1025": (lambda L, f, d8, u8, st: L.lhn_pck_accuracy(f[0], f[1], u8[0], f[2], fl(0.5), f[3], f[4], 2, 1025, st), "K <= 1024"),
        "refine_n0": (lambda L, f, d8, u8, st: L.lhn_heatmap_refine(f[0], f[1], 0, 3, 8, 8, 1, st), "lhn_heatmap_refine: bad shape"),
        "refine_w0": (lambda L, f, d8, u8, st: L.lhn_heatmap_refine(f[0], f[1], 2, 3, 8, 0, 0, st), "lhn_heatmap_refine: bad shape"),
        "transform_k0": (lambda L, f, d8, u8, st: L.lhn_transform_preds(f[0], f[1], f[2], f[3], 2, 0, 8, 8, 0, st), "lhn_transform_preds: bad shape"),
        "nms_h0": (lambda L, f, d8, u8, st: L.lhn_heatmap_nms(f[0], f[1], 2, 3, 0, 8, 3, st), "lhn_heatmap_nms: bad shape"),
        "nms_n0": (lambda L, f, d8, u8, st: L.lhn_heatmap_nms(f[0], f[1], 0, 3, 8, 8, 3, st), "lhn_heatmap_nms: bad shape"),
        "decode_n0": (lambda L, f, d8, u8, st: L.lhn_heatmap_decode(f[0], f[1], f[2], f[3], f[4], f[5], 0, 3, 8, 8, 1, st), "lhn_heatmap_decode: bad shape"),
        "dark_k0": (lambda L, f, d8, u8, st: L.lhn_heatmap_decode_dark(f[0], f[1], f[2], f[3], f[4], f[5], 2, 0, 8, 8, 3, st), "lhn_heatmap_decode_dark: bad shape"),
        "dark_udp_h0": (lambda L, f, d8, u8, st: L.lhn_heatmap_decode_dark_udp(f[0], f[1], f[2], f[3], f[4], f[5], 2, 3, 0, 8, 3, st), "lhn_heatmap_decode_dark_udp: bad shape"),
        "pck_n0": (lambda L, f, d8, u8, st: L.lhn_pck_accuracy(f[0], f[1], u8[0], f[2], fl(0.5), f[3], f[4], 0, 5, st), "lhn_pck_accuracy: bad shape"),
    }


REFUSE = _refuse_rows()


def run_refused(key, dev):
    """(status, message, every buffer handed to the call -- outputs and the pads behind them -- kept its prefill)."""
    fn, _ = REFUSE[key]
    n = 132 * 128 + PAD                      # room for the largest shape a row names
    f = [torch.full((n,), PREFILL, device=dev) for _ in range(6)]
    d8 = [torch.full((68 + PAD,), PREFILL, device=dev, dtype=torch.float64)]
    u8 = [torch.full((n,), 7, device=dev, dtype=torch.uint8)]
    rc = fn(_lib.lib(), [_lib.ptr(t) for t in f], [_lib.ptr(t) for t in d8], [_lib.ptr(t) for t in u8], _lib.stream())
    torch.cuda.synchronize()
    kept = all(bool((t == 7).all()) for t in f + d8 + u8)
    return rc, _lib.lib().lhn_last_error().decode(), kept


# ---------------------------------------------------------------- comparisons shared by the test and --check-reference
def ulp_close(a, b, ulps):
    """tests/test_heatmap_gpu.py's _ulp_close: np.spacing of a denormal is the denormal step, so a flushed denormal fails."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return bool(np.all(np.abs(a - b) <= ulps * np.spacing(np.maximum(np.abs(a), np.abs(b)))))


def denormals(t):
    return int(((t > 0) & (t < TINY)).sum())


def warp_ties(pre):
    """Pixels whose float64 value before rounding lies within WARP_MARGIN of a .5 tie ([N, 3, H, W] bool)."""
    return np.abs(pre - np.floor(pre) - 0.5) <= WARP_MARGIN


def dark_compared(group, g):
    """Maps of a DARK case that are compared.  UDP: the reference reads the neighbours of a (-1, -1) prediction through a flat index
    into the padded batch, which lands in the previous map; the kernel clamps into its own map.  The two agree where the previous map
    is non-positive as well (everything clipped to log(0.001)): the second of the two non-positive maps is compared, the first is not."""
    n = g["hm"].shape[0] * g["hm"].shape[1]
    keep = np.ones(n, bool)
    if group == "darku":
        keep[n - g["nneg"]] = False
    return keep.reshape(g["hm"].shape[:2])


# ---------------------------------------------------------------- input conditions (CPU)
def _check_reference():
    import time
    t0 = time.time()
    for grp, tab in GROUPS.items():
        for nm, c in tab.items():
            assert c.get("why"), f"{grp}:{nm}: no path / mistake named"
            g = inputs(grp, nm)
            r = reference(grp, nm, g)
            assert r, f"{grp}:{nm}: no outputs"
            note = ""
            if grp == "enc":
                dn = denormals(r["t1"])
                assert c["sigma"] != 1 or dn > 0, f"{grp}:{nm}: sigma = 1 without a denormal reference value"
                for m in (0, 1, 2):
                    assert np.isfinite(r[f"t{m}"]).all()
                assert 0.5 in r["w1"] and 1.0 in r["w1"]
                if c["set"] != "place":       # on / above / below every threshold: the weights flip inside each triple
                    rule = "w1" if c["set"] == "thr_unbiased" else "w0"
                    w = r[rule].reshape(-1)[:12].reshape(4, 3)
                    assert all(len(set(row)) == 2 for row in w.tolist()), f"{grp}:{nm}: a threshold triple does not flip: {w.tolist()}"
                note = f"denormals {dn}, weights {[int((r[f'w{m}'] > 0.5).sum()) for m in (0, 1, 2)]} of 14 on"
            elif grp == "amax":
                if c["kind"] == "props":
                    idx = r["index"].reshape(-1)
                    note = f"indices {idx.tolist()}"
                    assert (r["preds"].reshape(12, 2)[[6, 7, 9, 10]] == -1).all()
                else:
                    moved = (r["refined"] != g["coords"]).any(-1).sum()
                    assert np.isnan(r["refined"]).any() and moved > 0
                    note = f"{moved} of 27 predictions shifted"
            elif grp == "off":
                assert (r["refined"].reshape(20, 2)[17:] == -0.75).all() and (r["refined"].reshape(20, 2)[16] == np.array(g["coords"].reshape(20, 2)[16]) + 0.25).all()
            elif grp == "nms":
                kept = (r["hm"] != 0).mean()
                note = f"kept {kept:.2f}"
            elif grp == "simdr_enc":
                for k in ("tx", "ty"):        # arg-max is asked exactly: every visible row's maximum is a normal number and leads by 1e-3 relative
                    top = np.sort(r[k].reshape(10, -1), 1)[:, ::-1]
                    assert (top[[3, 9], 0] == 0).all(), "an invisible joint's vector is not zero"
                    vis = np.delete(top, [3, 9], 0)
                    assert (vis[:, 0] >= 1e-30).all() and (vis[:, 1] <= vis[:, 0] * (1 - 1e-3)).all(), f"{grp}:{nm} {k}: an ill-conditioned arg-max"
                ends = np.concatenate([r["tx"].argmax(2).reshape(-1), r["ty"].argmax(2).reshape(-1)])
                assert (ends == 0).sum() >= 4 and (r["tx"].argmax(2) == r["tx"].shape[2] - 1).any() and (r["ty"].argmax(2) == r["ty"].shape[2] - 1).any()
            elif grp == "simdr_loss":
                for a in "xy":
                    dd = np.abs(g["p" + a].astype(np.float64) - g["t" + a])
                    assert np.array_equal(dd, np.abs(g["d" + a]).astype(np.float64)), "p - t is not exact"
                    off1 = np.abs(dd[dd != 1] - 1).min()
                    assert off1 > 1e-3 and (dd == 1).any() and (dd > 1).any() and (dd < 1).any()
                r32 = reference(grp, nm, g, np.float32)
                note = f"margin of |d| from 1: {off1:.3f}; e32 " + " ".join(f"{k} {rel_err(r32[k], r[k]):.1e}" for k in r)
            elif grp == "loss":
                r32 = reference(grp, nm, g, np.float32)
                note = "e32 " + " ".join(f"{k} {rel_err(r32[k], r[k]):.1e}" for k in r)
                t = g["target"]
                assert c["kind"] != "half" or ((t == 0.5).any() and (t == np.nextafter(F32(0.5), F32(1))).any())
                assert c["kind"] != "nopos" or not (t > 0.5).any()
                assert c["kind"] != "allpos" or (t > 0.5).all()
            elif grp in ("dark", "darku"):
                r32 = reference(grp, nm, g, np.float32)
                keep = dark_compared(grp, g)
                e32 = float(np.abs(r32["hm_preds"] - r["hm_preds"])[keep].max())
                assert np.isfinite(r["hm_preds"][keep]).all()
                assert e32 <= 2e-3 / 3, f"{grp}:{nm}: e32 {e32:.2e} px: the Hessian is too close to singular, change the seed"
                npk = len(g["peaks"])
                assert np.array_equal(onp.get_max_preds(g["hm"])[0].reshape(-1, 2)[:npk], g["peaks"]), f"{grp}:{nm}: a peak is not where it was put"
                moved = (np.abs(r["hm_preds"].reshape(-1, 2)[:npk] - g["peaks"]) > 0).any(-1).sum()
                note = f"e32 {e32:.2e} px, {moved} of {npk} peaks refined"
            elif grp == "warp":
                worst = 0.0
                for n in range(4):
                    img = g["img"][n][:, ::-1] if c["flip"] and c["flip"][n] else g["img"][n]
                    p32 = _warp_pre32(img, g["center"][n], g["scale"][n], g["rot"][n], c["Wo"], c["Ho"], c["udp"])
                    worst = max(worst, float(np.abs(p32.transpose(2, 0, 1).astype(np.float64) - r["_pre"][n]).max()))
                share = float(warp_ties(r["_pre"]).any(1).mean())
                assert 3 * worst <= WARP_MARGIN, f"{grp}:{nm}: 3 x {worst:.3e} levels exceeds WARP_MARGIN"
                assert share <= WARP_CAP, f"{grp}:{nm}: {share:.3f} of the pixels within the margin of a tie"
                assert (r["_pre"][2] == 0).all() and (r["_pre"][[0, 1, 3]] > 0).any((1, 2, 3)).all()
                note = f"largest float32 change before rounding {worst:.3e} levels (margin {WARP_MARGIN:.1e}), excepted share {share:.4f}"
            elif grp == "hsv":
                assert c["n"] * c["h"] * c["w"] > 32 * 256 and c["h"] * c["w"] % (32 * 256) != 0
            print(f"{grp}:{nm}: ok" + (f" -- {note}" if note else ""))
    assert int(np.prod(LOSS["det_168x256"]["shape"])) > 16 * 1024
    print(f"{sum(len(t) for t in GROUPS.values())} cases, {len(REFUSE)} refusals, input conditions hold, {time.time() - t0:.1f} s")


def _print_instances():
    print("| group | case | kernels | path reached, mistake caught |\n|---|---|---|---|")
    for grp, tab in GROUPS.items():
        for nm, c in tab.items():
            print(f"| {grp} | {nm} | `{KERNELS[grp]}` | {c['why']} |")
    for key, (_, text) in REFUSE.items():
        print(f"| refuse | {key} | (none launched) | refused with \"{text}\", nothing written |")


if __name__ == "__main__":
    if sys.argv[1] == "--check-reference":
        _check_reference()
        sys.exit(0)
    if sys.argv[1] == "--instances":
        _print_instances()
        sys.exit(0)
    dst, reps, names = sys.argv[1], int(sys.argv[2]), sys.argv[3:]
    dev = torch.device("cuda:0")
    res = {}
    for full in names:
        grp, nm = full.split(":")
        g = inputs(grp, nm)
        for rep in range(reps):
            for k, v in run(grp, nm, dev, g).items():
                res[f"{full}/{rep}/{k}"] = v
    np.savez(dst, **res)
