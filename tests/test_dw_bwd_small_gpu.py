"""The small-map route of the 3x3 / dilation-1 depthwise backward (dw_bwd_route: maps of at most 256 pixels run the 8 x 16 tile
kernel k_dwk_bwd_lds with the BatchNorm-backward finalize folded into its prologue instead of the row kernel k_dw3_bwd_rows), through
lhn_conv_dw_bwd4 with the finalize source, so every case exercises the fold.

Cases: 8 x 8 at N = 3, 16 x 16 and 32 x 32 at N = 2 with 64 channels and the producer's BatchNorm sums (32 x 32 is above the size
rule and stays on the row kernel: its case tests that kernel through the same checks); 9 x 17 (one row and one column past a tile
edge) with the gate of y, the pooled gradient and an addend; 8 x 8 on channels [40, 80) of an 80-channel buffer with the gate of x,
accumulate and four replicas (the tail channel group, cvalid < 8, 40 BatchNorm channels: G = 25 groups); 12 x 12 with both addends.
Inputs and the float64 reference are those of tests/dw_bwd_cases.py, the finalize inputs those of tests/test_bwd_fin_consumer_gpu.py.

Per case: dx, dW and the producer's sums against float64 (the reference takes the coefficients a separate lhn_bn_bwd_finalize2
launch wrote) and the coefficients against the finalize's formula in float64, every element within max(2e-5, 3 x the float32 error
of the reference) -- the bar of tests/test_dw_bwd_gpu.py; no float outside the views changes; the row kernel (a child process with
LHN_DW_BWD_SMALL=0) meets the same bar and the two agree within it; the fold's coefficients, dgamma and dbeta equal the separate
launch's bit for bit; two runs of a child process under LHN_DETERMINISTIC=1 are bit-identical.

Run as a script it is the child: python tests/test_dw_bwd_small_gpu.py OUT.npz REPEATS NAME ..."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dw_bwd_cases as dc
from test_bwd_fin_consumer_gpu import FILL, _bn_inputs, _dw_new, _on, _same_bits, _separate

pytestmark = pytest.mark.gpu
TOL = 2e-5
# name: (dw_bwd_cases case, BatchNorm extras of the finalize source)
CASES = {
    "8_bns": (dc._case(3, 8, 8, 64, 0, 64, 1, "bns"), {}),
    "16_bns": (dc._case(2, 16, 16, 64, 0, 64, 1, "bns"), {"prior": True, "pscale": 0.5}),
    "32_bns": (dc._case(2, 32, 32, 64, 0, 64, 1, "bns"), {}),
    "9x17_gate_dpool_add": (dc._case(2, 9, 17, 64, 0, 64, 1, "ygate dpool add0"), {}),
    "8_tail40": (dc._case(2, 8, 8, 80, 40, 40, 1, "xgate acc nrep"), {"sc": 48, "nogamma": True}),
    "12_adds": (dc._case(2, 12, 12, 32, 0, 32, 1, "add0 add1"), {}),
}
for _n, (_c, _) in CASES.items():
    dc._ALL["dwsmall_" + _n] = _c


def _bn(case):
    n, h, w, cs, coff, c = dc._ALL["dwsmall_" + case][:6]
    return _bn_inputs(c, n * h * w, CASES[case][1], 11)


def _run(case, dev):
    """lhn_conv_dw_bwd4 with the finalize source on the case's inputs: the outputs of _dw_new, the coefficient table, dgamma, dbeta."""
    name = "dwsmall_" + case
    cs = dc._ALL[name][3]
    bn = _bn(case)
    b, coef = _on(bn, dev), torch.full((3, cs), FILL, device=dev)
    out = _dw_new(name, dev, dc.inputs(name), b, coef)
    out["coef"], out["dgamma"], out["dbeta"] = coef.cpu().numpy(), b["dgamma"].cpu().numpy(), b["dbeta"].cpu().numpy()
    out["fin_sums_ok"] = np.array(torch.equal(b["sums"], bn["sums"].to(dev)))
    return out


def _coef_reference(case, dtype):
    """A | B | C of the view's channels by the finalize's formula (include/lhn.h: lhn_bn_bwd_finalize2), in `dtype`."""
    n, h, w, cs, coff, c = dc._ALL["dwsmall_" + case][:6]
    bn = _bn(case)
    tot = bn["sums"].sum(0).numpy().astype(dtype)
    db, dg = tot[0, :c], tot[1, :c]
    mean, inv = (bn["save"][i, :c].numpy().astype(dtype) for i in range(2))
    gamma = bn["gamma"].numpy().astype(dtype) if bn["gamma"] is not None else np.ones(c, dtype)
    cnt = dtype(bn["count"])
    s = gamma * inv
    return np.stack([s, -s * inv * dg / cnt, -s * db / cnt + s * inv * mean * dg / cnt]).astype(np.float64)


def _child(tmp, env_extra, names, reps):
    out = os.path.join(str(tmp), "out.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out, str(reps)] + names, env=dict(os.environ, **env_extra),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return dict(np.load(out))


def _of(res, case, rep):
    pre = f"{case}/{rep}/"
    return {k[len(pre):]: v for k, v in res.items() if k.startswith(pre)}


@pytest.fixture(scope="module")
def rows_runs(dev, tmp_path_factory):
    """Every case on the row kernel (LHN_DW_BWD_SMALL=0), once per session."""
    return _child(tmp_path_factory.mktemp("dw_small_rows"), {"LHN_DW_BWD_SMALL": "0"}, list(CASES), 1)


@pytest.mark.parametrize("case", list(CASES))
def test_small_map_route_matches_float64_and_the_row_kernel(dev, rows_runs, case):
    name = "dwsmall_" + case
    n, h, w, cs, coff, c = dc._ALL[name][:6]
    g = dc.inputs(name)
    sep, coef_sep = _on(_bn(case), dev), torch.full((3, cs), FILL, device=dev)
    _separate(sep, coef_sep, cs, coff, c)
    got, rows = _run(case, dev), _of(rows_runs, case, 0)
    # the fold against the separate launch: bit for bit, the floats outside the BatchNorm's slice included
    _same_bits(got["coef"], coef_sep, f"{name} coef")
    _same_bits(got["dgamma"], sep["dgamma"], f"{name} dgamma")
    _same_bits(got["dbeta"], sep["dbeta"], f"{name} dbeta")
    assert bool((coef_sep[:, coff:coff + c] != FILL).all()) and bool((torch.cat([coef_sep[:, :coff], coef_sep[:, coff + c:]], 1) == FILL).all())
    gref = dict(g, coef=coef_sep.cpu())
    r64, r32 = dc.reference(name, gref), dc.reference(name, gref, torch.float32)
    r64["coef"], r32["coef"] = _coef_reference(case, np.float64), _coef_reference(case, np.float32)
    bad = []
    for k, ref in r64.items():
        bar = max(TOL, 3 * dc.rel_err(r32[k], ref))
        a, b = (got[k][:, coff:coff + c], rows[k][:, coff:coff + c]) if k == "coef" else (got[k], rows[k])
        assert a.shape == ref.shape == b.shape, f"{name} {k}: shapes {a.shape} {b.shape} {ref.shape}"
        e_new, e_rows, e_ab = dc.rel_err(a, ref), dc.rel_err(b, ref), dc.rel_err(a, b.astype(np.float64))
        print(f"dw_bwd_small {name} {k}: route {e_new:.3e}  rows {e_rows:.3e}  route vs rows {e_ab:.3e}  bar {bar:.3e}")
        bad += [f"{k} {what}: {e:.3e} > bar {bar:.3e}" for what, e in (("route", e_new), ("rows", e_rows), ("route vs rows", e_ab)) if not e <= bar]
    for path, res in (("route", got), ("rows", rows)):
        bad += [f"{path} {k}: floats that must keep their bits changed" for k, v in res.items() if k.endswith("_ok") and not bool(v)]
    assert not bad, f"{name}: " + "; ".join(bad)


def test_small_map_route_repeats_its_bits_in_deterministic_mode(dev, tmp_path):
    res = _child(tmp_path, {"LHN_DETERMINISTIC": "1"}, list(CASES), 2)
    for case in CASES:
        a, b = _of(res, case, 0), _of(res, case, 1)
        assert set(a) == set(b) and {"dx", "dw", "coef", "dgamma", "dbeta"} <= set(a)
        for k in a:
            _same_bits(a[k], b[k], f"{case} {k}")


if __name__ == "__main__":
    dst, reps, names = sys.argv[1], int(sys.argv[2]), sys.argv[3:]
    device = torch.device("cuda:0")
    out_all = {}
    for nm in names:
        for rep in range(reps):
            for key, val in _run(nm, device).items():
                out_all[f"{nm}/{rep}/{key}"] = val
    np.savez(dst, **out_all)
