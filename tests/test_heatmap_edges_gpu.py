"""Edge checks of csrc/k_heatmap.hip through the C ABI against the numpy / torch oracle: target encoding (biased, unbiased, UDP) at
non-square maps, every sigma class and the weight-zeroing thresholds; arg-max ties, NaN and infinities; refine, back-transform, peak
NMS, top-k candidates, PCK; the balanced-MSE and SimDR losses on both branches with non-unit weights and upstream gradients; DARK
decode around its Taylor guard; the affine warp over a grid that iterates; flip; HSV jitter and the loss under LHN_DETERMINISTIC=1
(grids capped at 2 CUs iterate); and the calls the library must refuse.  Bars are those of tests/test_heatmap_gpu.py for the same
quantity (exact, 1 / 2 ulp, 2.5e-7, 2e-3 px, one uint8 level on at most 5 % tie pixels) and the kernel bar max(2e-5, 3 x e32) of
tests/test_ew_pool_gpu.py for the losses.  profiles/heatmap_instances.md lists which case reaches which kernel and path."""
import os
import subprocess
import sys

import numpy as np
import pytest

import heatmap_cases as hc
from conftest import parity_record

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FLOOR = 2e-5        # the project's kernel-level floor (test_pw_gpu.FLOOR)
DARK_PX = 2e-3      # tests/test_heatmap_gpu.py: DARK coordinates, heat-map pixels

_REF = {}


def _reference(group, name):
    """(inputs, float64 reference, float32 reference or None); computed once per case and shared."""
    if (group, name) not in _REF:
        g = hc.inputs(group, name)
        r32 = hc.reference(group, name, g, np.float32) if group in ("loss", "simdr_loss", "dark", "darku") else None
        _REF[(group, name)] = (g, hc.reference(group, name, g), r32)
    return _REF[(group, name)]


def _same(a, b):
    """Equal in every element, NaN equal to NaN, same shape."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.array_equal(a, b, equal_nan=True))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _flags(got, bad):
    flags = [k for k in got if k.endswith("_ok")]
    assert flags, "no sentinel flags"
    bad += [f"{k}: elements outside the outputs changed" for k in flags if not bool(got[k])]


def _exact(group, name, got, keys, tag=""):
    _, ref, _ = _reference(group, name)
    bad = []
    for k in keys or [k for k in ref if not k.startswith("_")]:
        ok = _same(got[k], ref[k].astype(got[k].dtype) if got[k].dtype != ref[k].dtype else ref[k])
        parity_record(f"heatmap_edges/{tag}{group}_{name}", **{f"{k}_equal": ok})
        if not ok:
            bad.append(f"{k}: differs from the reference")
    _flags(got, bad)
    assert not bad, f"{tag}{group}:{name}: " + "; ".join(bad)


def _kernel_bar(group, name, got, tag=""):
    """max(FLOOR, 3 x e32) per output, every element, against the float64 reference."""
    _, r64, r32 = _reference(group, name)
    bad = []
    for k, ref in r64.items():
        assert got[k].shape == ref.shape, f"{group}:{name} {k}: shape {got[k].shape} vs {ref.shape}"
        err, e32 = hc.rel_err(got[k], ref), hc.rel_err(r32[k], ref)
        err = err if np.isfinite(err) else float("inf")
        bar = max(FLOOR, 3 * e32)
        parity_record(f"heatmap_edges/{tag}{group}_{name}", **{f"{k}_err": err, f"{k}_e32": e32, f"{k}_bar": bar})
        print(f"heatmap_edges {tag}{group}:{name} {k}: err {err:.3e} e32 {e32:.3e} bar {bar:.3e}")
        if not err <= bar:
            bad.append(f"{k}: err {err:.3e} > bar {bar:.3e}")
    _flags(got, bad)
    assert not bad, f"{tag}{group}:{name}: " + "; ".join(bad)


@pytest.mark.parametrize("name", list(hc.ENC))
def test_encode_edges(dev, name):
    """Weights exact; the exact-zero pattern of the biased and UDP maps exact; values 1 ulp (unbiased, UDP: float64 exp rounded once)
    and 2 ulp (biased: float32 expf).  np.spacing of a denormal is the denormal step: a flushed denormal fails."""
    g, ref, _ = _reference("enc", name)
    got = hc.run("enc", name, dev, g)
    bad, rec = [], {"ref_denormals": hc.denormals(ref["t1"]), "got_denormals": hc.denormals(got["t1"])}
    for mode, ulps in ((0, 2), (1, 1), (2, 1)):
        t, w = got[f"t{mode}"], got[f"w{mode}"]
        rec[f"w{mode}_equal"] = _same(w, ref[f"w{mode}"])
        rec[f"t{mode}_zero_pattern_equal"] = _same(t == 0, ref[f"t{mode}"] == 0)
        rec[f"t{mode}_within_{ulps}ulp"] = hc.ulp_close(t, ref[f"t{mode}"], ulps)
        rec[f"t{mode}_max_abs_diff"] = float(np.abs(t.astype(np.float64) - ref[f"t{mode}"]).max())
        if not rec[f"w{mode}_equal"]:
            bad.append(f"mode {mode}: weights differ")
        if mode != 1 and not rec[f"t{mode}_zero_pattern_equal"]:
            bad.append(f"mode {mode}: the zero pattern differs")
        if not rec[f"t{mode}_within_{ulps}ulp"]:
            bad.append(f"mode {mode}: values beyond {ulps} ulp (largest difference {rec[f't{mode}_max_abs_diff']:.3e})")
    parity_record(f"heatmap_edges/enc_{name}", **rec)
    print(f"heatmap_edges enc:{name}: {rec}")
    _flags(got, bad)
    assert not bad, f"enc:{name}: " + "; ".join(bad)


@pytest.mark.parametrize("name", list(hc.AMAX))
def test_argmax_decode_refine_transform_exact(dev, name):
    """np.argmax semantics (first maximum, NaN is the maximum): index, coordinates and maxima exact; post 1 / refine mode 0 exact
    against refine_default; the back-transform exact against transform_preds in float32."""
    g, _, _ = _reference("amax", name)
    _exact("amax", name, hc.run("amax", name, dev, g), None)


@pytest.mark.parametrize("name", list(hc.OFF))
def test_refine_offset_exact(dev, name):
    g, _, _ = _reference("off", name)
    _exact("off", name, hc.run("off", name, dev, g), None)


@pytest.mark.parametrize("name", list(hc.NMS))
def test_nms_bit_exact(dev, name):
    g, ref, _ = _reference("nms", name)
    got = hc.run("nms", name, dev, g)
    same = bool(np.array_equal(_bits(got["hm"]), _bits(ref["hm"])))                  # bits: -0.0 is not 0.0 here
    parity_record(f"heatmap_edges/nms_{name}", bits_equal=same)
    bad = [] if same else ["hm: differs from the reference in some bit"]
    _flags(got, bad)
    assert not bad, f"nms:{name}: " + "; ".join(bad)


@pytest.mark.parametrize("name", list(hc.TOPK))
def test_topk_exact(dev, name):
    g, _, _ = _reference("topk", name)
    _exact("topk", name, hc.run("topk", name, dev, g), None)


@pytest.mark.parametrize("name", list(hc.PCK))
def test_pck(dev, name):
    g, ref, _ = _reference("pck", name)
    got = hc.run("pck", name, dev, g)
    err = float(np.abs(got["acc"].astype(np.float64) - ref["acc"]).max())
    avg_err = abs(float(got["avg"]) - float(ref["avg"]))
    parity_record(f"heatmap_edges/pck_{name}", acc_err=err, avg_err=avg_err, cnt=int(got["cnt"]), cnt_ref=int(ref["cnt"]))
    bad = []
    if not err <= 1e-7:
        bad.append(f"accuracies differ by {err:.3e}")
    if not avg_err <= 1e-7:
        bad.append(f"average differs by {avg_err:.3e}")
    if int(got["cnt"]) != int(ref["cnt"]):
        bad.append(f"count {int(got['cnt'])} vs {int(ref['cnt'])}")
    _flags(got, bad)
    assert not bad, f"pck:{name}: " + "; ".join(bad)


@pytest.mark.parametrize("name", list(hc.LOSS))
def test_balanced_mse_matches_float64(dev, name):
    g, _, _ = _reference("loss", name)
    _kernel_bar("loss", name, hc.run("loss", name, dev, g))


@pytest.mark.parametrize("name", list(hc.SIMDR_ENC))
def test_simdr_encode(dev, name):
    g, ref, _ = _reference("simdr_enc", name)
    got = hc.run("simdr_enc", name, dev, g)
    bad, rec = [], {}
    for k in ("tx", "ty"):
        rec[f"{k}_err"] = float(np.abs(got[k].astype(np.float64) - ref[k]).max())
        rec[f"{k}_argmax_equal"] = _same(got[k].argmax(2), ref[k].argmax(2))
        if not rec[f"{k}_err"] <= 2.5e-7:
            bad.append(f"{k}: differs by {rec[f'{k}_err']:.3e}")
        if not rec[f"{k}_argmax_equal"]:
            bad.append(f"{k}: arg-max differs")
    parity_record(f"heatmap_edges/simdr_enc_{name}", **rec)
    _flags(got, bad)
    assert not bad, f"simdr_enc:{name}: " + "; ".join(bad)


@pytest.mark.parametrize("name", list(hc.SIMDR_LOSS))
def test_simdr_loss_matches_float64(dev, name):
    g, _, _ = _reference("simdr_loss", name)
    dd = np.abs(np.concatenate([g["dx"].reshape(-1), g["dy"].reshape(-1)]).astype(np.float64))
    parity_record(f"heatmap_edges/simdr_loss_{name}", d_margin_from_1=float(np.abs(dd[dd != 1] - 1).min()), d_equal_1=int((dd == 1).sum()))
    _kernel_bar("simdr_loss", name, hc.run("simdr_loss", name, dev, g))


@pytest.mark.parametrize("group,name", [(grp, n) for grp in ("dark", "darku") for n in hc.GROUPS[grp]])
def test_dark_decode(dev, group, name):
    """Maxima exact; coordinates within max(2e-3 px, 3 x e32) of the float64 oracle (the blur is "parity unpinned": a tolerance),
    e32 = what the float32 oracle loses against the float64 one; image coordinates within the same bar times the back-transform's
    pixel size (tests/test_heatmap_gpu.py asserts 2e-2 at a size of 4 to 6)."""
    g, r64, r32 = _reference(group, name)
    got = hc.run(group, name, dev, g)
    keep = hc.dark_compared(group, g)
    e32 = float(np.abs(r32["hm_preds"] - r64["hm_preds"])[keep].max())
    err = float(np.abs(got["hm_preds"].astype(np.float64) - r64["hm_preds"])[keep].max())
    err32 = float(np.abs(got["hm_preds"].astype(np.float64) - r32["hm_preds"])[keep].max())
    bar = max(DARK_PX, 3 * e32)
    px = (g["scale"].astype(np.float64) * 200 / (np.array(g["hm"].shape[:1:-1], np.float64) - (group == "darku")))[:, None, :]      # image pixels per heat-map pixel
    perr = float((np.abs(got["preds"].astype(np.float64) - r64["preds"]) / px)[keep].max())
    mv = _same(got["maxvals"], r64["maxvals"].astype(np.float32))
    parity_record(f"heatmap_edges/{group}_{name}", hm_preds_err=err, hm_preds_err_vs_float32_oracle=err32, e32=e32, bar=bar, preds_err_hm_px=perr, maxvals_equal=mv)
    print(f"heatmap_edges {group}:{name}: err {err:.3e} px (vs the float32 oracle {err32:.3e}) e32 {e32:.3e} bar {bar:.3e}; preds {perr:.3e}")
    bad = []
    if not mv:
        bad.append("maxima differ")
    if not err <= bar:
        bad.append(f"coordinates differ by {err:.3e} px > {bar:.3e}")
    if not perr <= bar:
        bad.append(f"image coordinates differ by {perr:.3e} heat-map px > {bar:.3e}")
    _flags(got, bad)
    assert not bad, f"{group}:{name}: " + "; ".join(bad)


@pytest.mark.parametrize("name", list(hc.WARP))
def test_affine_warp(dev, name):
    """1e-5 at every pixel, except pixels whose float64 value before rounding lies within WARP_MARGIN of a .5 tie: those may differ by
    one uint8 level, and at most 5 % of the pixels may be so excepted.  Joints to 1e-3 px."""
    g, ref, _ = _reference("warp", name)
    got = hc.run("warp", name, dev, g)
    diff = np.abs(got["out"].astype(np.float64) - ref["out"])
    tie = hc.warp_ties(ref["_pre"])
    level = (1.0 / 255 / np.array(hc.STD))[None, :, None, None]
    share, used = float(tie.any(1).mean()), float(((diff > 1e-5) & tie).any(1).mean())
    off_tie = float(np.where(tie, 0, diff).max())
    on_tie = float(np.where(tie, diff / level, 0).max())
    jerr = float(np.abs(got["joints"].astype(np.float64) - ref["joints"]).max())
    parity_record(f"heatmap_edges/warp_{name}", margin_levels=hc.WARP_MARGIN, excepted_share=share, excepted_and_different_share=used, err_off_ties=off_tie,
                  err_on_ties_levels=on_tie, joints_err=jerr)
    print(f"heatmap_edges warp:{name}: off ties {off_tie:.3e}, on ties {on_tie:.3f} levels, excepted share {share:.4f} (different: {used:.4f}), joints {jerr:.3e}")
    bad = []
    if not share <= hc.WARP_CAP:
        bad.append(f"{share:.3f} of the pixels excepted")
    if not off_tie <= 1e-5:
        bad.append(f"a pixel away from every tie differs by {off_tie:.3e}")
    if not on_tie <= 1 + 1e-3:
        bad.append(f"a tie pixel differs by {on_tie:.3f} levels")
    if not jerr < 1e-3:
        bad.append(f"joints differ by {jerr:.3e} px")
    _flags(got, bad)
    assert not bad, f"warp:{name}: " + "; ".join(bad)


@pytest.mark.parametrize("name", list(hc.FLIP))
def test_random_flip_exact(dev, name):
    g, _, _ = _reference("flip", name)
    _exact("flip", name, hc.run("flip", name, dev, g), None)


def test_deterministic_child(dev, tmp_path):
    """LHN_DETERMINISTIC=1 in a fresh process: the library reports 2 CUs, so the HSV grid is 32 blocks of 256 over 3 x 9360 pixels and
    the loss grids are 16 blocks over 43008 elements: both loops iterate.  HSV jitter equals the oracle in every bit; two runs of the loss
    agree bit for bit in value and gradient and meet the loss bar."""
    out = str(tmp_path / "out.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "heatmap_cases.py"), out, "2"] + hc.DET, env=dict(os.environ, LHN_DETERMINISTIC="1"),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = dict(np.load(out))
    for full in hc.DET:
        grp, nm = full.split(":")
        a, b = ({k[len(f"{full}/{rep}/"):]: v for k, v in res.items() if k.startswith(f"{full}/{rep}/")} for rep in (0, 1))
        assert a and a.keys() == b.keys()
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{full} {k}")
        if grp == "hsv":
            _exact(grp, nm, a, None, "deterministic/")
        else:
            _kernel_bar(grp, nm, a, "deterministic/")


def test_hsv_jitter_exact(dev):
    g, _, _ = _reference("hsv", "3x60x52")
    _exact("hsv", "3x60x52", hc.run("hsv", "3x60x52", dev, g), None)


@pytest.mark.parametrize("key", list(hc.REFUSE))
def test_refuses(dev, key):
    rc, err, untouched = hc.run_refused(key, dev)
    assert rc != 0 and hc.REFUSE[key][1] in err, f"{key}: status {rc}, error {err!r}"      # refused for the reason the row names
    assert untouched, f"{key}: a refused call wrote to a buffer"
