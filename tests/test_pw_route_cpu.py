"""CPU: the 1x1 route (lhn_conv_pw_route: host only, the functions every lhn_conv_pw_* entry itself asks) against a literal table
written down from the dispatch code as it stood before the route existed: every case of pw_cases.FWD / BWD, the case tuples of
tests/test_pw_bwd_wide_gpu.py, test_pw_bwd_narrow_gpu.py, test_pw_bwd_dzdead_gpu.py, test_head_stream_gpu.py and the 1x1 cases of
test_bwd_fin_consumer_gpu.py (repeated here: those modules need a GPU), by default and under every switch that changes the answer;
the refusals for lack of a kernel; the `split` flag of the case tables (dz holds dy after the call) against what the answer stores;
the tile rule of reader-side BatchNorm sums over every channel pair; one child process that sets LHN_PW_BWD_SPLIT=1."""
import os
import re
import subprocess
import sys

import pytest

import pw_cases as pc
from litehandnet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FINALIZE, REDUCE, DY = "lhn_bn_bwd_finalize2 + ", " + lhn_gate_bwd_reduce3", "k_dy_inplace + "
WIDE = {(128, 128): "k_pw_bwd_wr<128, 128, 32, 1, %s, false, 2>", (64, 128): "k_pw_bwd_wr<64, 128, 64, 1, %s, false, 2>",
        (128, 64): "k_pw_bwd_wr<128, 64, 64, 2, %s, false, 2>"}
NARROW = {(64, False): "k_pw_bwd_wr<64, 64, 64, 2, false, false, 2>", (64, True): "k_pw_bwd_wr<64, 64, 64, 2, false, true, 2>",
          (32, False): "k_pw_bwd_wr<32, 32, 128, 2, false, false, 3>", (32, True): "k_pw_bwd_wr<32, 32, 128, 2, false, true, 2>"}
# the narrow shapes on the fused kernel (LHN_PW_BWD_NARROW=0, LHN_PW_LDSW=1)
FUSED = {(64, False): "k_pw_bwd<64, 2, false, false>", (64, True): "k_pw_bwd<64, 2, false, true>",
         (32, False): "k_pw_bwd<32, 1, false, false>", (32, True): "k_pw_bwd<32, 1, false, true>"}
# the wide shapes on the three-launch path: LHN_PW_BWD_SPLIT=1 (data gradient on the register-W forward kernel), LHN_PW_LDSW=1 (k_kxk)
SPLIT = {(128, 128): ("k_pw_fwd_wr<128, 4, 1>", "k_kxk_wgrad<128, 4, 1, true>"), (64, 128): ("k_pw_fwd_wr<128, 2, 1>", "k_kxk_wgrad<64, 4, 1, true>"),
         (128, 64): ("k_pw_fwd_wr<64, 4, 1>", "k_kxk_wgrad<128, 2, 1, true>")}
SPLIT_LDSW = {(128, 128): "k_kxk<128, 4, 1, 1, true>", (64, 128): "k_kxk<128, 2, 1, 1, true>", (128, 64): "k_kxk<64, 4, 1, 1, true>"}
HEAD_OLD_FWD, HEAD_OLD_BWD = "k_pw_fwd<128, 1, 1>", "k_pw_bwd<128, 1, true, false> + k_bias_grad_nchw"


def _table(rows):
    return {case: kern for kern, cases in rows.items() for case in cases.split(", ")}


FWD = _table({
    "k_pw_fwd_wr<32, 1, 1>": "wr_32_32, big_32_32",
    "k_pw_fwd_wr<32, 2, 1>": "wr_32_64, tail_32_40",
    "k_pw_fwd_wr<32, 4, 1>": "wr_32_128, wr_tiny_32_128, tail_32_96",
    "k_pw_fwd_wr<64, 1, 1>": "wr_64_32",
    "k_pw_fwd_wr<64, 2, 1>": "wr_64_64, wr_tiny_64_64, view_64_64, big_64_64",
    "k_pw_fwd_wr<64, 4, 1>": "wr_64_128",
    "k_pw_fwd_wr<128, 2, 1>": "wr_128_64",
    "k_pw_fwd_wr<128, 4, 1>": "wr_128_128, big_128_128",
    "k_pw_fwd<128, 1, 1>": "view_128_32",                                  # no register-W instance for 128 -> <= 32
    "k_pw_fwd<128, 2, 1>": "s2_128_64_odd, s2_128_64_even",                # stride 2: the LDS-W kernel
    "k_pw_fwd<64, 2, 1>": "s2_64_64_odd, s2_64_64_even",
    "k_pw_fwd<32, 1, 1>": "s2_32_32_odd, s2_32_32_even, tail_20_20",       # partial K: the LDS-W kernel
    "k_pw_fwd<64, 4, 1>": "tail_40_80",
    "k_pw_fwd<128, 4, 1>": "tail_72_72",
    "k_pw_fwd<16, 1, 1>": "tail_12_24",
    "k_pw_fwd_wr<128, 4, 1> + k_pw_fwd_wr<32, 4, 1>": "slice_160_96",
    "k_pw_fwd_wr<128, 2, 1> x 2 + k_pw_fwd_wr<64, 2, 1>": "slice_320_40",
    "k_pw_fwd_wr<128, 2, 1> x 2 + k_pw_fwd<64, 2, 1>": "slice_300_60",     # the last K slice holds 44 of 64 channels
    "k_pw_fwd_wr<128, 2, 1> x 2": "slice_256_64",                          # K = 256 in one pass needs Cout % 128 == 0
    "k_pw_fwd_wr<64, 4, 1> x 2": "slice_64_256",
    "k_pw_fwd_wr<128, 4, 1> x 2": "slice_128_256",
    "k_pw_fwd<128, 1, 1> x 2": "slice_256_32, head_256_24",
    "k_pw_fwd_wr<256, 4, 1> x 2": "k256_256_256",
    "k_pw_fwd_wr<256, 4, 1>": "k256_256_128",
    "k_pw_fwd<64, 1, 1>": "head_64_24",
    "k_pw_fwd<32, 4, 1> x 2": "head_24_256",
    "k_pw_fwd_wr<64, 2, 3>": "ms_64_64_e1, ms_64_64_e2",
    "k_pw_fwd_wr<128, 4, 3>": "ms_128_128_e2",
    "k_pw_fwd<64, 2, 3>": "ms_64_64_e2_wmis",                              # weight pointer off a 16-byte boundary
})
FWD_LDSW = _table({       # every register-W launch on the LDS-W instance of the same tile
    "k_pw_fwd<32, 1, 1>": "wr_32_32, big_32_32",
    "k_pw_fwd<32, 2, 1>": "wr_32_64, tail_32_40",
    "k_pw_fwd<32, 4, 1>": "wr_32_128, wr_tiny_32_128, tail_32_96",
    "k_pw_fwd<64, 1, 1>": "wr_64_32",
    "k_pw_fwd<64, 2, 1>": "wr_64_64, wr_tiny_64_64, view_64_64, big_64_64",
    "k_pw_fwd<64, 4, 1>": "wr_64_128",
    "k_pw_fwd<128, 2, 1>": "wr_128_64",
    "k_pw_fwd<128, 4, 1>": "wr_128_128, big_128_128",
    "k_pw_fwd<128, 4, 1> + k_pw_fwd<32, 4, 1>": "slice_160_96",
    "k_pw_fwd<128, 2, 1> x 2 + k_pw_fwd<64, 2, 1>": "slice_320_40, slice_300_60",
    "k_pw_fwd<128, 2, 1> x 2": "slice_256_64",
    "k_pw_fwd<64, 4, 1> x 2": "slice_64_256",
    "k_pw_fwd<128, 4, 1> x 2": "slice_128_256, k256_256_128",
    "k_pw_fwd<128, 4, 1> x 4": "k256_256_256",
    "k_pw_fwd<64, 2, 3>": "ms_64_64_e1, ms_64_64_e2",
    "k_pw_fwd<128, 4, 3>": "ms_128_128_e2",
})
FWD_K256_OFF = _table({"k_pw_fwd_wr<128, 4, 1> x 4": "k256_256_256", "k_pw_fwd_wr<128, 4, 1> x 2": "k256_256_128"})

BWD = _table({
    NARROW[32, False]: "fused_32_32",
    "k_pw_bwd<32, 2, false, false>": "fused_32_64",
    "k_pw_bwd<32, 4, false, false>": "fused_32_128, full_32_128",
    "k_pw_bwd<64, 1, false, false>": "fused_64_32",
    NARROW[64, False]: "fused_64_64, full_64_64, nodx_64_64, big_64_64",
    "k_pw_bwd<128, 1, false, false>": "fused_128_32",
    "k_pw_bwd<32, 1, false, false>": "fused_20_20, s2_32_32",
    "k_pw_bwd<64, 4, false, false>": "fused_40_80",
    "k_pw_bwd<128, 4, false, false>": "fused_72_72",
    "k_pw_bwd<128, 2, false, false> + k_pw_bwd<32, 2, false, false>": "fused_160_40",
    WIDE[128, 128] % "true": "nodx_128_128, split_128_128, big_128_128",
    "k_pw_bwd<128, 2, false, false>": "s2_128_64",
    NARROW[64, True]: "bns_64_64_16, bns_64_64_odd",
    "k_pw_bwd<32, 2, false, true>": "bns_32_64_16, bns_32_64_odd",
    "k_pw_bwd<64, 1, false, true>": "bns_64_32_16, bns_64_32_odd",
    "k_pw_bwd<128, 1, true, false> + k_bias_grad_nchw + k_pw_bwd<128, 1, true, false>": "head_256_24",
    "k_pw_bwd<64, 1, true, false> + k_bias_grad_nchw": "head_64_24",
    WIDE[64, 128] % "true": "split_64_128",
    WIDE[128, 64] % "true": "split_128_64",
    DY + "k_pw_fwd_wr<256, 4, 1> x 2 + k_kxk_wgrad<128, 4, 1, true> x 2": "split_256_256",
    DY + "k_pw_fwd_wr<128, 4, 1> x 2 + k_kxk_wgrad<128, 4, 1, true> x 2": "split_256_128",
    DY + "k_pw_fwd_wr<256, 4, 1> + k_kxk_wgrad<128, 4, 1, true>": "split_128_256",
    DY + "k_pw_fwd_wr<64, 4, 1> x 2 + k_kxk_wgrad<128, 2, 1, true> x 2": "split_256_64",
    DY + "k_pw_fwd_wr<128, 2, 1> x 2 + k_kxk_wgrad<64, 4, 1, true>": "split_64_256",
    DY + "k_pw_fwd_wr<32, 4, 1> x 2 + k_kxk_wgrad<128, 1, 1, true> x 2": "split_256_32",
})
BWD_LDSW = _table({       # no register-W kernel: the narrow shapes on k_pw_bwd, every data gradient of the split path on k_kxk
    FUSED[32, False]: "fused_32_32",
    FUSED[64, False]: "fused_64_64, full_64_64, nodx_64_64, big_64_64",
    FUSED[64, True]: "bns_64_64_16, bns_64_64_odd",
    DY + "k_kxk_wgrad<128, 4, 1, true>": "nodx_128_128",
    DY + "k_kxk<128, 2, 1, 1, true> + k_kxk_wgrad<64, 4, 1, true>": "split_64_128",
    DY + "k_kxk<64, 4, 1, 1, true> + k_kxk_wgrad<128, 2, 1, true>": "split_128_64",
    DY + "k_kxk<128, 4, 1, 1, true> + k_kxk_wgrad<128, 4, 1, true>": "split_128_128, big_128_128",
    DY + "k_kxk<128, 4, 1, 1, true> x 2 + k_kxk_wgrad<128, 4, 1, true> x 2": "split_256_256",
    DY + "k_kxk<128, 4, 1, 1, true> + k_kxk_wgrad<128, 4, 1, true> x 2": "split_256_128",
    DY + "k_kxk<128, 4, 1, 1, true> x 2 + k_kxk_wgrad<128, 4, 1, true>": "split_128_256",
    DY + "k_kxk<64, 4, 1, 1, true> + k_kxk_wgrad<128, 2, 1, true> x 2": "split_256_64",
    DY + "k_kxk<128, 2, 1, 1, true> x 2 + k_kxk_wgrad<64, 4, 1, true>": "split_64_256",
    DY + "k_kxk<32, 4, 1, 1, true> + k_kxk_wgrad<128, 1, 1, true> x 2": "split_256_32",
})
BWD_NARROW_OFF = _table({FUSED[32, False]: "fused_32_32", FUSED[64, False]: "fused_64_64, full_64_64, nodx_64_64, big_64_64",
                         FUSED[64, True]: "bns_64_64_16, bns_64_64_odd"})
BWD_SPLIT_ON = _table({
    DY + "k_kxk_wgrad<128, 4, 1, true>": "nodx_128_128",
    DY + "k_pw_fwd_wr<128, 2, 1> + k_kxk_wgrad<64, 4, 1, true>": "split_64_128",
    DY + "k_pw_fwd_wr<64, 4, 1> + k_kxk_wgrad<128, 2, 1, true>": "split_128_64",
    DY + "k_pw_fwd_wr<128, 4, 1> + k_kxk_wgrad<128, 4, 1, true>": "split_128_128, big_128_128",
})
SWITCHED = (("fwd", FWD_LDSW, {"ldsw": True}), ("fwd", FWD_K256_OFF, {"k256": False}), ("bwd", BWD_LDSW, {"ldsw": True}),
            ("bwd", BWD_NARROW_OFF, {"narrow": False}), ("bwd", BWD_SPLIT_ON, {"split": True}))

# ---------------------------------------------------------------- the GPU modules' cases: name -> (pw_cases case, further features)
MODULE = {}
# tests/test_pw_bwd_wide_gpu.py
_PIX = {"tail": (2, 5, 7), "tiny": (1, 3, 3), "tiles": (3, 8, 8)}
for _ci, _co in ((128, 128), (64, 128), (128, 64)):
    for _tag, _nhw in _PIX.items():
        MODULE[f"wide_{_ci}_{_co}_{_tag}"] = (pc._case(_ci, _co, _nhw, "split dbias"), 0)
    MODULE[f"wide_{_ci}_{_co}_loop"] = (pc._case(_ci, _co, (5, 8, 8), "split"), 0)
for _nm, _fl, _kw in (("store", "split", {}), ("acc", "split acc", {}), ("nodx", "split nodx", {}), ("nrep1", "split dbias acc", {"nrep": 1}),
                      ("xgate", "split xgate", {}), ("views", "split views dbias", {}), ("ygate_dpool", "split ygate dpool", {})):
    MODULE[f"wide_128_128_{_nm}"] = (pc._case(128, 128, _PIX["tail"], _fl, **_kw), 0)
# tests/test_pw_bwd_narrow_gpu.py
_PIX = {"tiny": (1, 3, 3), "tail": (2, 5, 7), "tiles": (3, 8, 8), "loop": (5, 8, 8)}
_PIX128 = {"tail128": (2, 10, 10), "tiles128": (6, 8, 8), "loop128": (10, 8, 8)}
for _c in (64, 32):
    for _tag, _nhw in dict(_PIX, **(_PIX128 if _c == 32 else {})).items():
        MODULE[f"narrow_{_c}_{_c}_{_tag}"] = (pc._case(_c, _c, _nhw, "dbias"), 0)
        MODULE[f"narrow_{_c}_{_c}_bns_{_tag}"] = (pc._case(_c, _c, _nhw, "bns"), 0)
    for _nm, _fl, _kw in (("store", "", {}), ("acc", "acc", {}), ("nodx", "nodx", {}), ("nrep1", "dbias acc", {"nrep": 1}), ("xgate", "xgate", {}),
                          ("views", "views dbias", {}), ("ygate_dpool", "ygate dpool", {})):
        MODULE[f"narrow_{_c}_{_c}_{_nm}"] = (pc._case(_c, _c, _PIX["tail"], _fl, **_kw), 0)
# tests/test_pw_bwd_dzdead_gpu.py: each case with LHN_PW_BWD_DZ_DEAD, the _fin ones with a finalize source
for (_ci, _co), _nhw in {(128, 128): (3, 5, 7), (64, 128): (2, 9, 9), (128, 64): (2, 9, 9)}.items():
    MODULE[f"dzdead_{_ci}_{_co}_dbias"] = (pc._case(_ci, _co, _nhw, "dbias"), pc.F_DZ_DEAD)
    MODULE[f"dzdead_{_ci}_{_co}_acc"] = (pc._case(_ci, _co, _nhw, "acc"), pc.F_DZ_DEAD)
    MODULE[f"dzdead_{_ci}_{_co}_fin"] = (pc._case(_ci, _co, _nhw, ""), pc.F_DZ_DEAD | pc.F_FIN)
    MODULE[f"dzdead_{_ci}_{_co}_fin_acc_dbias"] = (pc._case(_ci, _co, _nhw, "acc dbias"), pc.F_DZ_DEAD | pc.F_FIN)
MODULE["dzdead_128_128_views_fin"] = (pc._case(128, 128, (3, 5, 7), "xgate ygate dpool dbias views"), pc.F_DZ_DEAD | pc.F_FIN)
# the 1x1 cases of tests/test_bwd_fin_consumer_gpu.py, each with a finalize source
for _nm, _c in {"64_64_8": pc._case(64, 64, (2, 8, 8)), "32_32_8": pc._case(32, 32, (2, 8, 8)), "128_128_16": pc._case(128, 128, (2, 16, 16), "split"),
                "64_128_16": pc._case(64, 128, (2, 16, 16), "split dbias"), "128_64_16": pc._case(128, 64, (2, 16, 16), "split acc"),
                "64_64_9x7": pc._case(64, 64, (2, 9, 7), "acc"), "32_32_9x7": pc._case(32, 32, (2, 9, 7), ""), "32_32_bns": pc._case(32, 32, (2, 8, 8), "bns"),
                "64_64_views": pc._case(64, 64, (2, 8, 8), "xgate ygate dpool acc views"), "32_64_fallback": pc._case(32, 64, (2, 8, 8), "dbias")}.items():
    MODULE["fin_" + _nm] = (_c, pc.F_FIN)
# tests/test_head_stream_gpu.py (the gate-sum cases carry `slices`: kernel_of sets LHN_PW_F_GATESUM for them)
_PIX = {"one": (3, 8, 8), "two": (2, 8, 16), "straddle": (3, 6, 6), "multi": (5, 16, 16), "tail": (1, 10, 10)}
HEAD_FWD, _BF = {}, "nchw dbias xgate views"
for _tag, _nhw in _PIX.items():
    HEAD_FWD[f"head_fwd_{_tag}"] = pc._case(128, 21, _nhw, "xtab xgate xview nchw bias nostats")
    MODULE[f"head_bwd_{_tag}"] = (pc._case(128, 21, _nhw, _BF), 0)
for _co in (4, 32):
    HEAD_FWD[f"head_fwd_c{_co}"] = pc._case(128, _co, _PIX["two"], "xtab xgate xview nchw bias nostats")
    MODULE[f"head_bwd_c{_co}"] = (pc._case(128, _co, _PIX["two"], _BF), 0)
MODULE["head_bwd_acc"] = (pc._case(128, 21, _PIX["tail"], _BF + " acc", nrep=1), 0)
MODULE["head_bwd_nodx"] = (pc._case(128, 21, _PIX["two"], _BF + " nodx"), 0)
MODULE["head_bwd_big"] = (pc._case(128, 21, (9, 64, 64), _BF, nrep=16), 0)
for _nm, (_nhw, _sl) in {"head_gs0_one": (_PIX["one"], ()), "head_gs1_two": (_PIX["two"], ((64, 64),)), "head_gs2_multi": (_PIX["multi"], ((0, 32), (64, 64))),
                         "head_gs2_straddle": (_PIX["straddle"], ((0, 32), (64, 64))), "head_gs2_runs": ((520, 8, 16), ((0, 32), (64, 64)))}.items():
    MODULE[_nm] = (pc._case(128, 21, _nhw, "nchw dbias xgate", slices=_sl), 0)
pc._ALL["fwd"].update({"route_" + k: v for k, v in HEAD_FWD.items()})
pc._ALL["bwd"].update({"route_" + k: v[0] for k, v in MODULE.items()})


def _want_module(name, ldsw=False, narrow=True, split=False, head_stream=True, deterministic=False):
    """The expected launches of a MODULE case, written out per family."""
    c, extra = MODULE[name]
    ci, co, f = c["cin"], c["cout"], c["flags"]
    fin = FINALIZE if extra & pc.F_FIN else ""
    if (ci, co) in WIDE:
        if ldsw:
            return fin + DY + ("" if "nodx" in f else SPLIT_LDSW[ci, co] + " + ") + SPLIT[ci, co][1]
        if split:
            return fin + DY + ("" if "nodx" in f else SPLIT[ci, co][0] + " + ") + SPLIT[ci, co][1]
        return WIDE[ci, co] % ("false" if extra & pc.F_DZ_DEAD else "true")          # the finalize rides in the prologue
    if ci == co and ci in (64, 32):
        return fin + FUSED[ci, "bns" in f] if (ldsw or not narrow) else NARROW[ci, "bns" in f]
    if (ci, co) == (32, 64):
        return fin + "k_pw_bwd<32, 2, false, false>"
    assert ci == 128 and co <= 32 and "nchw" in f
    gs, hw = "slices" in c, c["nhw"][1] * c["nhw"][2]
    if ldsw or not head_stream or (gs and (hw % 64 or deterministic)):
        return HEAD_OLD_BWD + (REDUCE if gs else "")
    return "k_head_bwd<true>" if gs else "k_head_bwd<false>"


def test_forward_tables():
    assert set(FWD) == set(pc.FWD)
    for nm, want in FWD.items():
        assert pc.kernel_of("fwd", nm) == want, nm
        assert pc.kernel_of("fwd", nm, narrow=False, split=True, head_stream=False, deterministic=True) == want, nm
        assert pc.kernel_of("fwd", nm, ldsw=True) == FWD_LDSW.get(nm, want), nm
        assert pc.kernel_of("fwd", nm, k256=False) == FWD_K256_OFF.get(nm, want), nm


def test_backward_tables():
    assert set(BWD) == set(pc.BWD)
    for nm, want in BWD.items():
        assert pc.kernel_of("bwd", nm) == want, nm
        assert pc.kernel_of("bwd", nm, k256=False, head_stream=False, deterministic=True) == want, nm
        assert pc.kernel_of("bwd", nm, ldsw=True) == BWD_LDSW.get(nm, want), nm
        assert pc.kernel_of("bwd", nm, narrow=False) == BWD_NARROW_OFF.get(nm, want), nm
        assert pc.kernel_of("bwd", nm, split=True) == BWD_SPLIT_ON.get(nm, want), nm


@pytest.mark.parametrize("name", sorted(MODULE))
def test_module_cases(name):
    extra = MODULE[name][1]
    for kw in ({}, {"ldsw": True}, {"k256": False}, {"narrow": False}, {"split": True}, {"head_stream": False}, {"deterministic": True}):
        want = _want_module(name, **{k: v for k, v in kw.items() if k != "k256"})
        assert pc.kernel_of("bwd", "route_" + name, extra, **kw) == want, kw


def test_module_cases_spelled_out():
    """One literal answer per family, so that _want_module's own composition is pinned too."""
    ask = lambda nm, **kw: pc.kernel_of("bwd", "route_" + nm, MODULE[nm][1], **kw)      # noqa: E731
    assert ask("wide_64_128_tail") == "k_pw_bwd_wr<64, 128, 64, 1, true, false, 2>"
    assert ask("wide_128_128_nodx", split=True) == "k_dy_inplace + k_kxk_wgrad<128, 4, 1, true>"
    assert ask("dzdead_128_64_fin") == "k_pw_bwd_wr<128, 64, 64, 2, false, false, 2>"
    assert ask("dzdead_128_64_fin", split=True) == "lhn_bn_bwd_finalize2 + k_dy_inplace + k_pw_fwd_wr<64, 4, 1> + k_kxk_wgrad<128, 2, 1, true>"
    assert ask("dzdead_128_128_fin", ldsw=True) == "lhn_bn_bwd_finalize2 + k_dy_inplace + k_kxk<128, 4, 1, 1, true> + k_kxk_wgrad<128, 4, 1, true>"
    assert ask("narrow_32_32_bns_tail128") == "k_pw_bwd_wr<32, 32, 128, 2, false, true, 2>"
    assert ask("fin_32_32_bns", narrow=False) == "lhn_bn_bwd_finalize2 + k_pw_bwd<32, 1, false, true>"
    assert ask("fin_64_64_views") == "k_pw_bwd_wr<64, 64, 64, 2, false, false, 2>"
    assert ask("fin_32_64_fallback") == "lhn_bn_bwd_finalize2 + k_pw_bwd<32, 2, false, false>"
    assert ask("head_bwd_straddle") == "k_head_bwd<false>"
    assert ask("head_gs2_multi") == "k_head_bwd<true>"
    assert ask("head_gs2_multi", deterministic=True) == "k_pw_bwd<128, 1, true, false> + k_bias_grad_nchw + lhn_gate_bwd_reduce3"
    assert ask("head_gs2_straddle") == "k_pw_bwd<128, 1, true, false> + k_bias_grad_nchw + lhn_gate_bwd_reduce3"
    assert ask("head_bwd_c32", head_stream=False) == "k_pw_bwd<128, 1, true, false> + k_bias_grad_nchw"


def test_head_forward_cases():
    for nm in HEAD_FWD:
        assert pc.kernel_of("fwd", "route_" + nm) == "k_head_fwd", nm
        assert pc.kernel_of("fwd", "route_" + nm, k256=False, narrow=False, split=True, deterministic=True) == "k_head_fwd", nm
        assert pc.kernel_of("fwd", "route_" + nm, head_stream=False) == HEAD_OLD_FWD, nm
        assert pc.kernel_of("fwd", "route_" + nm, ldsw=True) == HEAD_OLD_FWD, nm
        assert pc.kernel_of("fwd", "route_" + nm, pc.F_UNALIGNED) == HEAD_OLD_FWD, nm


def test_no_kernel_is_null():
    assert pc.kernel_of("fwd", "extra_32_32") is None
    for nm in ("bns_large", "bns_stride2"):
        assert pc.kernel_of("bwd", nm) is None, nm
    # refused for another reason than the lack of a kernel: the query does not look at those arguments
    for kind, nm in (("fwd", "extras_stride2"), ("fwd", "sum_out_alone"), ("bwd", "s2_store"), ("bwd", "bns_xgate")):
        assert pc.kernel_of(kind, nm) is not None, nm
    # sums whose TILES reach 64 x 128 although Cin * Cout does not
    sw, ask = pc.SW_K256 | pc.SW_BWD_NARROW | pc.SW_HEAD_STREAM, _lib.lib().lhn_conv_pw_route
    assert ask(1, 2, 8, 8, 40, 80, 1, 0, 0, pc.F_BNSUM, sw) is None
    # ... but with an NCHW gradient the call runs the NCHW instance, which takes no sums, and is accepted by the channel product
    assert ask(1, 2, 8, 8, 40, 80, 1, 0, 0, pc.F_BNSUM | pc.F_NCHW, sw) == b"k_pw_bwd<64, 4, true, false>"
    assert ask(1, 2, 8, 8, 128, 24, 1, 0, 0, pc.F_BNSUM | pc.F_NCHW | pc.F_DBIAS, pc.SW_K256) == b"k_pw_bwd<128, 1, true, false> + k_bias_grad_nchw"
    assert ask(1, 2, 8, 8, 128, 64, 1, 0, 0, pc.F_BNSUM | pc.F_NCHW, sw) is None
    # a stride no call accepts
    for stride in (0, 3, -1):
        assert ask(1, 2, 8, 8, 64, 64, stride, 0, 0, 0, sw) is None and ask(0, 2, 8, 8, 64, 64, stride, 0, 0, 0, sw) is None


def test_split_flag_is_what_the_route_stores():
    """`split` in a case's flags (dz holds dy after the call) exactly when the launches store dy over dz: k_dy_inplace, or a DYST = true
    instance of k_pw_bwd_wr.  The dz-dead module's cases run with LHN_PW_BWD_DZ_DEAD and carry no flag."""
    stores = lambda r: "k_dy_inplace" in r or re.search(r"k_pw_bwd_wr<\d+, \d+, \d+, \d+, true,", r) is not None      # noqa: E731
    for nm, c in pc.BWD.items():
        assert ("split" in c["flags"]) == stores(pc.kernel_of("bwd", nm)), nm
    for nm, (c, extra) in MODULE.items():
        assert ("split" in c["flags"]) == stores(pc.kernel_of("bwd", "route_" + nm, extra)), nm


def test_bn_sums_tile_rule():
    """The rule the plan compiler used to carry (plan.py: _can_add_bn_sums), written out: stride 1, both sides <= 128, tiles below
    64 x 128.  The route with the sums feature has a kernel exactly there."""
    L = _lib.lib()
    for stride in (1, 2):
        for cin in range(4, 257, 4):
            for cout in range(4, 257, 4):
                ci_t = 32 if cin <= 32 else 64 if cin <= 64 else 128
                nto = (cout + 31) // 32
                nto = 4 if nto == 3 else nto
                rule = stride == 1 and cin <= 128 and cout <= 128 and ci_t * nto * 32 < 64 * 128
                for sw in (pc.SW_K256 | pc.SW_BWD_NARROW | pc.SW_HEAD_STREAM, pc.SW_LDSW):
                    got = L.lhn_conv_pw_route(1, 2, 8, 8, cin, cout, stride, 0, 0, pc.F_BNSUM | pc.F_DX_ACC * (stride == 2), sw)
                    assert (got is not None) == rule, (stride, cin, cout, sw)


def test_environment_is_read():
    """switches = -1: as the process read them.  Here nothing is set; a child sets LHN_PW_BWD_SPLIT=1."""
    ask = ("import sys; sys.path.insert(0, %r); from litehandnet_amd import _lib; L = _lib.lib(); "
           "print(L.lhn_conv_pw_route(1, 2, 8, 8, 128, 128, 1, 0, 0, 0, -1).decode()); "
           "print(L.lhn_conv_pw_route(0, 2, 8, 8, 256, 128, 1, 0, 0, 2, -1).decode())" % ROOT)
    env = {k: v for k, v in os.environ.items() if not k.startswith(("LHN_PW_", "LHN_HEAD_", "LHN_DETERMINISTIC"))}
    plain = subprocess.run([sys.executable, "-c", ask], env=env, capture_output=True, text=True, check=True).stdout.split("\n")[:2]
    assert plain == [WIDE[128, 128] % "true", "k_pw_fwd_wr<256, 4, 1>"]
    child = subprocess.run([sys.executable, "-c", ask], env=dict(env, LHN_PW_BWD_SPLIT="1"), capture_output=True, text=True, check=True)
    assert child.stdout.split("\n")[:2] == [DY + "k_pw_fwd_wr<128, 4, 1> + k_kxk_wgrad<128, 4, 1, true>", "k_pw_fwd_wr<256, 4, 1>"]
