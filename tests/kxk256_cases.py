"""Cases of the dense 3x3 convolution with a side of 256 channels (lhn_conv_kxk_fwd / lhn_conv_kxk_bwd, csrc/k_conv_kxk.hip), run
through the C ABI with the harness of tests/kxk_cases.py: its runners, references, prefills and `*_ok` guards.  The tables below are
registered in that module's lookup dictionary (`_ALL`) at import and nowhere else, so its own tables -- and the tests parametrised
over them -- stay as they are.  Imported by tests/test_kxk256_gpu.py; as a script (a child process with its own environment):
    python tests/kxk256_cases.py OUT.npz REPEATS fwd:NAME bwd:NAME ...
    python tests/kxk256_cases.py --check-reference        (CPU only)

What runs where: profiles/kxk_instances.md (printed by `python tests/kxk_cases.py --instances` from kxk_cases.kernel_of, which serves the
tables registered here too).  K = 256 runs as two 128-channel slices per tap inside k_kxk<256, NT, MODE, 9>, 256 features as blocks of at
most 4 tiles of 32 on gridDim.y, the weight gradient once per 128-channel input slice; every case with a side of 256 is on the plain
path (dz := dy in place first), whatever LHN_PLAIN says.
The `fwd:fin_256_256` pseudo-case is pair-shaped with a fused BatchNorm finalize (run_fwd_fin).

Is the bar max(2e-5, 3 * e32) meaningful at K = 2,304?  --check-reference prints e32 (torch's float32 CPU run against float64,
relative to the largest magnitude) per case and output: 7.1e-8 .. 2.5e-6 over all cases here (y 4.1e-7..2.5e-6, dx 8.9e-8..1.9e-6,
dw 2.0e-7..2.5e-6, dz <= 1e-7, statistics <= 4.1e-7), so every bar is the 2e-5 floor, while a dropped K half moves y by 0.78 and
the table and gate of the wrong half by 0.50 of its largest magnitude (checked there too, on view_256_256: `half-K`, `swapped`)."""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kxk_cases as kc  # noqa: E402
from dw_fwd_cases import EPS, MOMENTUM, SLOPE, STAT_REPLICAS, TICKET_WORDS, BnFin  # noqa: E402
from kxk_cases import PREFILL, _case, _lib, _outside, _view, rel_err  # noqa: E402,F401

PAIRS = [(256, 256), (256, 128), (256, 64), (256, 32), (128, 256), (64, 256), (32, 256)]
MT = [(256, 256), (128, 256), (256, 128), (256, 64), (64, 256)]      # (the last two reach NT = 2 in the deterministic child)

# ---------------------------------------------------------------- forward table (flags as in kxk_cases)
FWD = {}
for _ci, _co in PAIRS:
    FWD[f"pair_{_ci}_{_co}"] = _case(_ci, _co, (3, 9, 13), "xtab")                  # 351 px: no multiple of 128, images straddle tiles
FWD["tiny_256_256"] = _case(256, 256, (1, 5, 7))                                    # 35 px: under one tile
FWD["view_256_256"] = _case(256, 256, (2, 12, 20), "xtab xgate xview yview")        # x = channels [64, 320), y = [32, 288): each K half its own table / gate
FWD["tail_256_40"] = _case(256, 40, (2, 9, 11), "xtab")                             # the last feature tile is 8 channels wide, K sliced
FWD["s2_256_256_odd"] = _case(256, 256, (2, 11, 11), "xtab", stride=2)
FWD["s2_256_256_even"] = _case(256, 256, (1, 8, 10), "xtab", stride=2)
for _ci, _co in MT:
    FWD[f"mt_{_ci}_{_co}"] = _case(_ci, _co, (3, 24, 25), "xtab")                   # 1,800 px = 15 tiles: deterministic child NT = 4 (gridDim.y = 2 at 256 features)
# 37,249 px = 292 tiles of 128 pixels on a forward grid of lhn_num_cus() * 1 = 256 workgroups (x gridDim.y = 2, NT = 4): 36 workgroups
# per y take a second tile.  (The sliced instances keep the LDS of <128, NT>: one workgroup per CU.)
FWD["big_256_256"] = _case(256, 256, (1, 193, 193), "xtab")

# ---------------------------------------------------------------- backward table
BWD = {}
for _i, (_ci, _co) in enumerate(PAIRS):
    BWD[f"pair_{_ci}_{_co}"] = _case(_ci, _co, (3, 9, 13), "acc" if _i % 2 else "")
for _i, (_ci, _co) in enumerate(PAIRS):
    BWD[f"rep1_{_ci}_{_co}"] = _case(_ci, _co, (3, 9, 13), "" if _i % 2 else "acc", nrep=1)
BWD["tiny_256_256"] = _case(256, 256, (1, 5, 7))
for _e, _nhw in (("odd", (2, 11, 11)), ("even", (1, 8, 10))):
    BWD[f"s2_256_256_{_e}_store"] = _case(256, 256, _nhw, "", stride=2)             # variant A's encoder BasicBlock: dgrad by pixel parity, K sliced
    BWD[f"s2_256_256_{_e}_acc"] = _case(256, 256, _nhw, "acc", stride=2)
for _ci, _co in MT:
    BWD[f"mt_{_ci}_{_co}"] = _case(_ci, _co, (3, 24, 25), "acc" if _ci == _co else "")
BWD["cosplit_256_256"] = _case(256, 256, (4, 31, 33), "")                           # 4,092 px = 64 wgrad tiles = 16 * nrep: exclusive flush, 8 groups
BWD["nocosplit_256_256"] = _case(256, 256, (5, 29, 29), "acc")                      # 66 tiles: one past the threshold, atomic flush, 2 groups of 4 tiles
BWD["full_256_256"] = _case(256, 256, (2, 16, 19), "ygate dpool acc views")
BWD["nodx_256_256"] = _case(256, 256, (2, 8, 8), "nodx")
BWD["big_256_256"] = _case(256, 256, (1, 193, 193), "", nrep=16)                    # dgrad: 292 tiles on 256 x 2 workgroups; wgrad atomic flush

# refused before the first launch, nothing written.  256 -> 48 is a backward refusal only: the forward takes a partial last
# feature tile at every K (tail_256_40 here, tail_32_48 in kxk_cases), the backward has no K = 48 dgrad.
_R = "unsupported channels"
FWD_REFUSE = {f"r_{ci}_{co}": _case(ci, co, (2, 8, 8), "xtab", refuse=_R) for ci, co in ((512, 256), (256, 512), (256, 96), (192, 256))}
BWD_REFUSE = {f"r_{ci}_{co}": _case(ci, co, (2, 8, 8), "", refuse=_R) for ci, co in ((512, 256), (256, 512), (256, 96), (192, 256), (256, 48))}

TABLES = {"fwd": FWD, "bwd": BWD}
for _kind, _tabs in (("fwd", (FWD, FWD_REFUSE)), ("bwd", (BWD, BWD_REFUSE))):
    for _t in _tabs:
        for _k, _v in _t.items():
            assert _k not in kc._ALL[_kind], _k
            kc._ALL[_kind][_k] = _v


# ---------------------------------------------------------------- forward with the fused BatchNorm finalize
FIN_CASE = "pair_256_256"       # 3 tiles x gridDim.y = 8: 24 workgroups draw tickets, one finalizes


def fin_inputs(seed=7):
    g = kc.inputs("fwd", FIN_CASE, seed)
    c = kc._ALL["fwd"][FIN_CASE]["cout"]
    g["gamma"], g["beta"] = 1 + 0.3 * kc._rand((c,), seed + 20), 0.2 * kc._rand((c,), seed + 21)
    g["rmean"], g["rvar"] = 0.1 * kc._rand((c,), seed + 22), 1 + 0.2 * kc._rand((c,), seed + 23).abs()
    return g


def run_fwd_fin(dev, g=None):
    """lhn_conv_kxk_fwd with fin != NULL on FIN_CASE: the table (scale | shift | slope), mean | invstd, running statistics, and the
    ticket words after the launch (`tickets_ok`: the top word holds min(blocks, 32), the 32 group words sum to the block count --
    every workgroup of gridDim.x * gridDim.y drew exactly one ticket, so exactly one was last)."""
    c = kc._ALL["fwd"][FIN_CASE]
    (n, h, w), cin, cout = c["nhw"], c["cin"], c["cout"]
    g = g or fin_inputs()
    d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in g.items()}
    L, st = _lib.lib(), _lib.stream()
    vx = _view(d["x"], 0, cin, d.get("xtab"))
    y = torch.full((n, h, w, cout), PREFILL, device=dev)
    vy = _view(y, 0, cout)
    sbuf = torch.zeros(STAT_REPLICAS, 2, cout, dtype=torch.float64, device=dev)
    scr = torch.full((9 * cout * cin + kc.SLACK,), PREFILL, device=dev)
    ycs, ycoff = cout + 16, 8
    fb = {"counter": torch.zeros(TICKET_WORDS, dtype=torch.int32, device=dev), "table": torch.full((3, ycs), PREFILL, device=dev),
          "save": torch.full((2, cout), PREFILL, device=dev), "rmean": d["rmean"].clone(), "rvar": d["rvar"].clone(),
          "nbt": torch.full((1,), 5, dtype=torch.int64, device=dev)}
    fin = BnFin()
    fin.counter, fin.gamma, fin.beta = fb["counter"].data_ptr(), d["gamma"].data_ptr(), d["beta"].data_ptr()
    fin.running_mean, fin.running_var, fin.num_batches_tracked = fb["rmean"].data_ptr(), fb["rvar"].data_ptr(), fb["nbt"].data_ptr()
    fin.table, fin.save_mean_invstd, fin.count = fb["table"].data_ptr(), fb["save"].data_ptr(), float(n * h * w)
    fin.cstride, fin.coff, fin.C, fin.eps, fin.momentum, fin.slope = ycs, ycoff, cout, EPS, MOMENTUM, SLOPE
    fin.conv_bias = None
    rc = L.lhn_conv_kxk_fwd(C.byref(vx), _lib.ptr(d["w"]), C.byref(vy), _lib.ptr(sbuf), 1, C.byref(fin), _lib.ptr(scr), st)
    torch.cuda.synchronize()
    _lib.check(rc, "kxk fwd fin")
    tab = fb["table"][:, ycoff:ycoff + cout].cpu().numpy()
    cnt = fb["counter"].cpu().numpy().astype(np.int64)
    ntiles = (n * h * w + 127) // 128
    blocks = {ntiles * s for s in (2, 4, 8)}                 # gridDim.y is the library's choice: 2, 4 or 8
    return {"y": y.cpu().numpy(), "fin_scale": tab[0], "fin_shift": tab[1], "fin_slope": tab[2],
            "fin_mean": fb["save"][0].cpu().numpy(), "fin_invstd": fb["save"][1].cpu().numpy(),
            "fin_rmean": fb["rmean"].cpu().numpy(), "fin_rvar": fb["rvar"].cpu().numpy(), "fin_nbt": fb["nbt"].cpu().numpy(),
            "table_outside_ok": np.array(bool((_outside(fb["table"], ycoff, cout) == PREFILL).all())),
            "tickets_ok": np.array(int(cnt[1:].sum()) in blocks and int(cnt[0]) == min(int(cnt[1:].sum()), 32)),
            "tickets": cnt}


def reference_fwd_fin(g=None, dtype=torch.float64):
    g = g or fin_inputs()
    y = torch.from_numpy(kc.reference_fwd(FIN_CASE, g, dtype)["y"]).to(dtype)
    cnt = y.shape[0] * y.shape[1] * y.shape[2]
    mean, var = y.mean((0, 1, 2)), y.var((0, 1, 2), unbiased=False)
    invstd = 1 / torch.sqrt(var + EPS)
    sc = g["gamma"].to(dtype) * invstd
    out = {"y": y, "fin_scale": sc, "fin_shift": g["beta"].to(dtype) - mean * sc, "fin_slope": torch.full_like(sc, SLOPE),
           "fin_mean": mean, "fin_invstd": invstd,
           "fin_rmean": (1 - MOMENTUM) * g["rmean"].to(dtype) + MOMENTUM * mean,
           "fin_rvar": (1 - MOMENTUM) * g["rvar"].to(dtype) + MOMENTUM * var * cnt / (cnt - 1)}
    return {k: v.double().numpy() for k, v in out.items()}


# ---------------------------------------------------------------- CPU self-check
def _check_reference():
    import time
    t0, lo, hi = time.time(), 1.0, 0.0
    for kind, tab in TABLES.items():
        for nm in tab:
            if nm.startswith("big_"):
                continue                                     # (the same operation as pair_256_256 on a larger map; seconds of float64 each)
            g = kc.inputs(kind, nm)
            assert g["seed"] == 7, f"{kind}:{nm} needed seed {g['seed']}"
            r64, r32 = kc.reference(kind, nm, g), kc.reference(kind, nm, g, torch.float32)
            for k in r64:
                assert np.isfinite(r64[k]).all(), f"{kind}:{nm} {k}"
                e = rel_err(r32[k], r64[k])
                lo, hi = min(lo, e), max(hi, e)
                print(f"{kind}:{nm} {k}: e32 {e:.2e} bar {max(2e-5, 3 * e):.2e}")
    # what a wrong K half would look like, on the view case: the table / gate values of the halves differ, a dropped half and
    # swapped halves of table and gate both sit orders of magnitude over the bar
    nm = "view_256_256"
    g = kc.inputs("fwd", nm)
    xcs, xcoff = kc.geometry("fwd", nm)[:2]
    a, b = slice(xcoff, xcoff + 128), slice(xcoff + 128, xcoff + 256)
    assert not torch.equal(g["xtab"][:, a], g["xtab"][:, b]) and not torch.equal(g["xgate"][:, a], g["xgate"][:, b])
    r64 = kc.reference_fwd(nm, g)["y"]
    gh = dict(g, w=g["w"].clone())
    gh["w"][:, 128:] = 0
    gs = dict(g, xtab=g["xtab"].clone(), xgate=g["xgate"].clone())
    gs["xtab"][:, b], gs["xgate"][:, b] = g["xtab"][:, a], g["xgate"][:, a]
    eh, es = rel_err(kc.reference_fwd(nm, gh)["y"], r64), rel_err(kc.reference_fwd(nm, gs)["y"], r64)
    print(f"half-K {eh:.2e}  swapped {es:.2e}")
    assert eh > 1e-2 and es > 1e-2 and 3 * hi < 1e-4
    gf = fin_inputs()
    f64, f32 = reference_fwd_fin(gf), reference_fwd_fin(gf, torch.float32)
    print("fin e32", {k: f"{rel_err(f32[k], f64[k]):.1e}" for k in f64})
    print(f"{sum(len(t) for t in TABLES.values())} cases, e32 {lo:.1e} .. {hi:.1e}, {time.time() - t0:.1f} s")


if __name__ == "__main__":
    if sys.argv[1] == "--check-reference":
        _check_reference()
        sys.exit(0)
    dst, reps, names = sys.argv[1], int(sys.argv[2]), sys.argv[3:]
    dev = torch.device("cuda:0")
    res = {}
    for full in names:
        kind, nm = full.split(":")
        g = kc.inputs(kind, nm)
        for r in range(reps):
            for k, v in kc.run(kind, nm, dev, g).items():
                res[f"{full}/{r}/{k}"] = v
    np.savez(dst, **res)
