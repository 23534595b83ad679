"""Cases of the dense 3x3 convolution at the channel counts of mynet at width 160 -- 160 -> 160 (BasicBlock) and 40 -> 40 (the stem's
branch and the inner convolution of BottleNeck, 40 = 160 / 4) -- through lhn_conv_kxk_fwd / lhn_conv_kxk_bwd (csrc/k_conv_kxk.hip), run
with the harness of tests/kxk_cases.py: its runners, references, prefills and `*_ok` guards.  The tables below are registered in that
module's lookup dictionary (`_ALL`) at import and nowhere else, as tests/kxk256_cases.py does, so the older tables -- and the tests
parametrised over them -- stay as they are.  Imported by tests/test_kxk160_gpu.py; as a script (a child process with its own
environment):
    python tests/kxk160_cases.py OUT.npz REPEATS fwd:NAME bwd:NAME ...
    python tests/kxk160_cases.py --check-reference        (CPU only)
    python tests/kxk160_cases.py --instances              (CPU only: prints profiles/kxk160_instances.md)

K = 160 runs as five 32-channel slices per tap inside k_kxk<160, NT, MODE, 9> (forward and plain data gradient), 160 features as five
tiles of 32 in one block (NT = 5) or one per block on gridDim.y = 5, the weight gradient as a 128-channel and a 32-channel input slice
with Cout = 160 on five or three groups; every 160 case is on the plain path whatever LHN_PLAIN says.  K = 40 runs on the 64-channel
LDS images with channels [40, 64) zero; 40 * 40 < 4096, so its default backward forms dy on the fly and LHN_PLAIN=1 or a pooled
gradient makes it plain.  Which case launches what: profiles/kxk160_instances.md.
`fwd:fin_160_160` is pair-shaped with a fused BatchNorm finalize (run_fwd_fin); `fwd:concat_40_40` is the stem's branch: stride 2, y
is channels [0, 40) of an 80-wide buffer whose other half keeps its bits (run_fwd_concat).

--check-reference prints e32 (torch's float32 CPU run against float64, relative to the largest magnitude) per case and output, and
shows that the bar max(2e-5, 3 * e32) sees a dropped 32-channel K slice at 160 and a dropped tail [32, 40) at 40 (view_*: x sits
inside a wider buffer, so every slice and the tail have their own table and gate values next to foreign floats)."""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kxk_cases as kc  # noqa: E402
from dw_fwd_cases import EPS, MOMENTUM, SLOPE, STAT_REPLICAS, TICKET_WORDS, BnFin  # noqa: E402
from kxk_cases import PREFILL, _case, _lib, _outside, _view, rel_err  # noqa: E402,F401

WIDTHS = (40, 160)

# ---------------------------------------------------------------- forward table (flags as in kxk_cases)
FWD = {}
for _c in WIDTHS:
    FWD[f"pair_{_c}_{_c}"] = _case(_c, _c, (3, 9, 13), "xtab")                      # 351 px: no multiple of 128, images straddle tiles
    FWD[f"tiny_{_c}_{_c}"] = _case(_c, _c, (1, 5, 7))                               # 35 px: under one tile
    FWD[f"view_{_c}_{_c}"] = _case(_c, _c, (2, 12, 20), "xtab xgate xview yview")   # x = channels [64, 64 + C), y = [32, 32 + C)
    FWD[f"s2_{_c}_{_c}_odd"] = _case(_c, _c, (2, 11, 11), "xtab", stride=2)
    FWD[f"s2_{_c}_{_c}_even"] = _case(_c, _c, (1, 8, 10), "xtab", stride=2)
    FWD[f"mt_{_c}_{_c}"] = _case(_c, _c, (3, 24, 25), "xtab")                       # 15 tiles: the deterministic child loops (NT = 5 / NT = 2)
# 37,249 px = 292 tiles, fewer than 2 * 256: one feature tile per block on gridDim.y = 5, more tiles than resident workgroups
FWD["big_160_160"] = _case(160, 160, (1, 193, 193), "xtab")
# NT = 5 (five tiles in one block, what the workload's 64 x 64 maps at batch 64 run) needs 2 * CUs tiles: 512 on the device, 4 in the
# deterministic child, where the view / full / mt cases above and these stride-2 maps reach it (DET below)
FWD["s2mt_160_160"] = _case(160, 160, (2, 33, 33), "xtab", stride=2)                 # 578 output px = 5 tiles

# ---------------------------------------------------------------- backward table
BWD = {}
for _i, _c in enumerate(WIDTHS):
    BWD[f"pair_{_c}_{_c}"] = _case(_c, _c, (3, 9, 13), "acc" if _i else "")
    BWD[f"pairacc_{_c}_{_c}"] = _case(_c, _c, (3, 9, 13), "" if _i else "acc")
    BWD[f"rep1_{_c}_{_c}"] = _case(_c, _c, (3, 9, 13), "acc", nrep=1)
    BWD[f"rep1store_{_c}_{_c}"] = _case(_c, _c, (3, 9, 13), "", nrep=1)
    BWD[f"tiny_{_c}_{_c}"] = _case(_c, _c, (1, 5, 7))
    BWD[f"full_{_c}_{_c}"] = _case(_c, _c, (2, 16, 19), "ygate dpool acc views")
    for _e, _nhw in (("odd", (2, 11, 11)), ("even", (1, 8, 10))):
        BWD[f"s2_{_c}_{_c}_{_e}_store"] = _case(_c, _c, _nhw, "", stride=2)         # data gradient by pixel parity
        BWD[f"s2_{_c}_{_c}_{_e}_acc"] = _case(_c, _c, _nhw, "acc", stride=2)
    BWD[f"mt_{_c}_{_c}"] = _case(_c, _c, (3, 24, 25), "acc")
    BWD[f"nodx_{_c}_{_c}"] = _case(_c, _c, (2, 8, 8), "nodx")
BWD["fly_40_40"] = _case(40, 40, (2, 16, 19), "xgate ygate acc views")              # dy on the fly: the default path at 40
BWD["dpool_40_40"] = _case(40, 40, (2, 16, 19), "dpool")                            # a pooled gradient forces the plain path below 4096
# the route chunks the weight gradient (pixel chunks = gradient replicas, exclusive flush) while wgrad tiles <= 16 * nrep
BWD["cosplit_160_160"] = _case(160, 160, (4, 31, 33), "")                           # 4,092 px = 64 tiles = 16 * nrep: five groups of one tile
BWD["nocosplit_160_160"] = _case(160, 160, (5, 29, 29), "acc")                      # 66 tiles: one past it, three groups of two tiles, atomic flush
BWD["big_160_160"] = _case(160, 160, (1, 193, 193), "", nrep=16)                    # dgrad one tile per block on 292 tiles; wgrad atomic flush
BWD["s2mt_160_160"] = _case(160, 160, (2, 33, 33), "acc", stride=2)                 # 2,178 input px: the parity classes have 2 .. 3 tiles each

# refused before the first launch, nothing written: every pair with a side of 160 but 160 -> 160, every pair that would need the
# padded K = 40 but 40 -> 40.  (64 -> 40 forward is older than width 160 and stays: kxk_cases tail_64_40.)
_R = "unsupported channels"
# ... and five feature tiles exist for 160 alone: 64 -> 144 (which a five-tile rule without the pair would serve on small maps)
_MIXED = ((40, 160), (160, 40), (40, 64), (40, 32), (160, 128), (128, 160), (160, 256), (32, 160), (64, 144), (144, 64))
FWD_REFUSE = {f"r_{ci}_{co}": _case(ci, co, (2, 8, 8), "xtab", refuse=_R) for ci, co in _MIXED}
BWD_REFUSE = {f"r_{ci}_{co}": _case(ci, co, (2, 8, 8), "", refuse=_R) for ci, co in _MIXED + ((64, 40),)}

TABLES = {"fwd": FWD, "bwd": BWD}
for _kind, _tabs in (("fwd", (FWD, FWD_REFUSE)), ("bwd", (BWD, BWD_REFUSE))):
    for _t in _tabs:
        for _k, _v in _t.items():
            assert _k not in kc._ALL[_kind], _k
            kc._ALL[_kind][_k] = _v

# what the deterministic child runs twice (tests/test_kxk160_gpu.py): on 2 CUs every 160 case from 4 tiles on is NT = 5, so five tiles
# in one block meet views, gates, a pooled gradient and the stride-2 paths there; FIN_DET is the fused finalize at gridDim.y = 1
DET = (["fwd:mt_40_40", "fwd:mt_160_160", "fwd:view_160_160", "fwd:s2mt_160_160", "bwd:mt_160_160", "bwd:full_160_160", "bwd:s2mt_160_160"] +
       [f"bwd:{_n}" for _n, _c in BWD.items() if _c["cin"] == 40])
FIN_DET = "mt_160_160"

# the old refusals that tests pin (kxk_cases / kxk256_cases): (Cin, Cout, backward only)
OLD_REFUSALS = ((48, 64, False), (64, 96, False), (128, 96, False), (96, 64, False), (192, 256, False), (256, 96, False), (256, 48, True),
                (512, 256, False), (256, 512, False), (512, 512, False))


# ---------------------------------------------------------------- the stem's concatenation: 40 -> 40, stride 2, y = [0, 40) of 80
CONCAT_CASE, CONCAT_CS = "s2_40_40_odd", 80


def run_fwd_concat(dev, g=None):
    """lhn_conv_kxk_fwd on CONCAT_CASE with y as channels [0, 40) of an 80-wide buffer (my_pelee_stem: the pooled branch owns the other
    half): y, the statistics, and `y_outside_ok`: channels [40, 80) keep the bits they were prefilled with."""
    c = kc._ALL["fwd"][CONCAT_CASE]
    (n, h, w), cin, cout, s = c["nhw"], c["cin"], c["cout"], c["stride"]
    ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
    g = g or kc.inputs("fwd", CONCAT_CASE)
    d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in g.items()}
    L, st = _lib.lib(), _lib.stream()
    vx = _view(d["x"], 0, cin, d.get("xtab"))
    other = kc._rand((n, ho, wo, CONCAT_CS), 99).to(dev)
    y = other.clone()
    vy = _view(y, 0, cout)
    sbuf = torch.zeros(32, 2, cout, dtype=torch.float64, device=dev)
    scr = torch.full((9 * cout * cin + kc.SLACK,), PREFILL, device=dev)
    rc = L.lhn_conv_kxk_fwd(C.byref(vx), _lib.ptr(d["w"]), C.byref(vy), _lib.ptr(sbuf), s, None, _lib.ptr(scr), st)
    torch.cuda.synchronize()
    _lib.check(rc, "kxk fwd concat")
    tot = sbuf.sum(0).cpu().numpy()
    return {"y": y[..., :cout].cpu().numpy(), "stats_sum": tot[0], "stats_sq": tot[1],
            "y_outside_ok": np.array(torch.equal(y[..., cout:], other[..., cout:])),
            "wt_ok": np.array(torch.equal(scr[:-kc.SLACK].view(9, cout, cin), d["w"].view(cout, cin, 9).permute(2, 0, 1)) and
                              bool((scr[-kc.SLACK:] == PREFILL).all()))}


# ---------------------------------------------------------------- forward with the fused BatchNorm finalize
FIN_CASE = "pair_160_160"       # 3 tiles x gridDim.y = 5: 15 workgroups draw tickets, one finalizes


def fin_inputs(seed=7, case=None):
    g = kc.inputs("fwd", case or FIN_CASE, seed)
    c = kc._ALL["fwd"][case or FIN_CASE]["cout"]
    g["gamma"], g["beta"] = 1 + 0.3 * kc._rand((c,), seed + 20), 0.2 * kc._rand((c,), seed + 21)
    g["rmean"], g["rvar"] = 0.1 * kc._rand((c,), seed + 22), 1 + 0.2 * kc._rand((c,), seed + 23).abs()
    return g


def _fin_cus():
    return 2 if os.environ.get("LHN_DETERMINISTIC") == "1" else 256


def run_fwd_fin(dev, g=None, case=None):
    """lhn_conv_kxk_fwd with fin != NULL on FIN_CASE (or `case`), as kxk256_cases.run_fwd_fin: table, mean | invstd, running statistics
    and the ticket words (`tickets_ok`: the top word holds min(blocks, 32), the 32 group words sum to the block count -- every
    workgroup of gridDim.x * gridDim.y drew exactly one ticket, so exactly one was last).  gridDim.y is what the route answers for
    this process (5, or 1 with NT = 5); gridDim.x is the tile count, or in the deterministic child any count up to it."""
    case = case or FIN_CASE
    c = kc._ALL["fwd"][case]
    (n, h, w), cin, cout = c["nhw"], c["cin"], c["cout"]
    g = g or fin_inputs(case=case)
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
    route = kc.kernel_of("fwd", case, cus=_fin_cus())
    gy = int(route.split(" y")[1]) if " y" in route else 1
    assert ("<160, 5," in route) == (gy == 1), route
    blocks = {ntiles * gy} if _fin_cus() == 256 else {gx * gy for gx in range(1, ntiles + 1)}
    return {"y": y.cpu().numpy(), "fin_scale": tab[0], "fin_shift": tab[1], "fin_slope": tab[2],
            "fin_mean": fb["save"][0].cpu().numpy(), "fin_invstd": fb["save"][1].cpu().numpy(),
            "fin_rmean": fb["rmean"].cpu().numpy(), "fin_rvar": fb["rvar"].cpu().numpy(), "fin_nbt": fb["nbt"].cpu().numpy(),
            "table_outside_ok": np.array(bool((_outside(fb["table"], ycoff, cout) == PREFILL).all())),
            "tickets_ok": np.array(int(cnt[1:].sum()) in blocks and int(cnt[0]) == min(int(cnt[1:].sum()), 32)),
            "tickets": cnt, "grid_y": np.array(gy)}


def reference_fwd_fin(g=None, dtype=torch.float64, case=None):
    g = g or fin_inputs(case=case)
    y = torch.from_numpy(kc.reference_fwd(case or FIN_CASE, g, dtype)["y"]).to(dtype)
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
def dropped_k(name, lo, hi):
    """How far y of a forward case moves, relative to its peak, when input channels [lo, hi) of w are zeroed."""
    g = kc.inputs("fwd", name)
    r64 = kc.reference_fwd(name, g)["y"]
    gh = dict(g, w=g["w"].clone())
    gh["w"][:, lo:hi] = 0
    return rel_err(kc.reference_fwd(name, gh)["y"], r64)


def _check_reference():
    import time
    t0, lo, hi = time.time(), 1.0, 0.0
    for kind, tab in TABLES.items():
        for nm in tab:
            if nm.startswith("big_"):
                continue                                     # (the same operation as pair_160_160 on a larger map; seconds of float64)
            g = kc.inputs(kind, nm)
            assert g["seed"] == 7, f"{kind}:{nm} needed seed {g['seed']}"
            r64, r32 = kc.reference(kind, nm, g), kc.reference(kind, nm, g, torch.float32)
            for k in r64:
                assert np.isfinite(r64[k]).all(), f"{kind}:{nm} {k}"
                e = rel_err(r32[k], r64[k])
                lo, hi = min(lo, e), max(hi, e)
                print(f"{kind}:{nm} {k}: e32 {e:.2e} bar {max(2e-5, 3 * e):.2e}")
    # what a dropped K slice / a dropped tail would look like, on the view cases: orders of magnitude over the bar
    for sl in range(5):
        e = dropped_k("view_160_160", 32 * sl, 32 * sl + 32)
        print(f"view_160_160 without K slice {sl}: {e:.2e}")
        assert e > 1e-2
    e = dropped_k("view_40_40", 32, 40)
    print(f"view_40_40 without channels [32, 40): {e:.2e}")
    assert e > 1e-2 and 3 * hi < 1e-4
    for nm in ("view_160_160", "view_40_40"):                # the slices' table and gate values differ
        g = kc.inputs("fwd", nm)
        xcoff, cin = kc.geometry("fwd", nm)[1], kc._ALL["fwd"][nm]["cin"]
        a, b = slice(xcoff, xcoff + 8), slice(xcoff + cin - 8, xcoff + cin)
        assert not torch.equal(g["xtab"][:, a], g["xtab"][:, b]) and not torch.equal(g["xgate"][:, a], g["xgate"][:, b])
    gf = fin_inputs()
    f64, f32 = reference_fwd_fin(gf), reference_fwd_fin(gf, torch.float32)
    print("fin e32", {k: f"{rel_err(f32[k], f64[k]):.1e}" for k in f64})
    print(f"{sum(len(t) for t in TABLES.values())} cases, e32 {lo:.1e} .. {hi:.1e}, {time.time() - t0:.1f} s")


def _instances():
    """profiles/kxk160_instances.md, in the format of profiles/kxk_instances.md."""
    print("# Dense 3x3 convolution kernels at 40 and 160 channels: which test case launches what\n")
    print("The answers of `lhn_conv_kxk_route` (`include/lhn.h`: host only, the route functions `lhn_conv_kxk_fwd` / `lhn_conv_kxk_bwd` ask) for\n"
          "`FWD` / `BWD` of `tests/kxk160_cases.py`, printed by `python tests/kxk160_cases.py --instances`; `tests/test_kxk160_route_cpu.py`\n"
          "holds every case against the harness's own rules.  Spelling as in `profiles/kxk_instances.md`; behind a 160-channel input the weight\n"
          "gradient is two launches, a 128-channel and a 32-channel input slice.")
    for kind, title in (("fwd", "Forward"), ("bwd", "Backward")):
        base = {nm: kc.kernel_of(kind, nm) for nm in TABLES[kind]}
        for setting, kw in kc.SETTINGS:
            got = {nm: kc.kernel_of(kind, nm, **kw) for nm in TABLES[kind]}
            rows = {}
            for nm, k in got.items():
                if not kw or k != base[nm]:
                    rows.setdefault(k, []).append(nm)
            if not rows:
                continue
            print(f"\n## {title}, {setting}" + (": the cases that change their launches" if kw else "") + "\n\n| launches | cases |\n|---|---|")
            for k, names in rows.items():
                print(f"| `{k}` | {', '.join(names)} |")
    print("\n## Refused for lack of a kernel (the query answers NULL)\n")
    print(", ".join(f"{kind}:{nm}" for kind, t in (("fwd", FWD_REFUSE), ("bwd", BWD_REFUSE)) for nm in t if kc.kernel_of(kind, nm) is None))


if __name__ == "__main__":
    if sys.argv[1] == "--check-reference":
        _check_reference()
        sys.exit(0)
    if sys.argv[1] == "--instances":
        _instances()
        sys.exit(0)
    dst, reps, names = sys.argv[1], int(sys.argv[2]), sys.argv[3:]
    dev = torch.device("cuda:0")
    res = {}
    for full in names:
        kind, nm = full.split(":")
        fin = nm.startswith("fin@")                           # fwd:fin@CASE: the forward with the fused finalize on CASE
        g = fin_inputs(case=nm[4:]) if fin else kc.inputs(kind, nm)
        for r in range(reps):
            for k, v in (run_fwd_fin(dev, g, nm[4:]) if fin else kc.run(kind, nm, dev, g)).items():
                res[f"{full}/{r}/{k}"] = v
    np.savez(dst, **res)
