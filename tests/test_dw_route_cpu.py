"""CPU: the depthwise route (lhn_conv_dw_route: host only, the function lhn_conv_dw_fwd3 / lhn_conv_dw_bwd4 themselves ask) against
a literal table: every table of profiles/dw_instances.md as written down before the route existed, the cases of
tests/test_dw_bwd_small_gpu.py and the depthwise cases of tests/test_bwd_fin_consumer_gpu.py with a finalize source (their tuples
are repeated here: those modules need a GPU), the refusals for lack of a kernel, and one child process that sets LHN_DW_GATHER=1."""
import os
import subprocess
import sys

import pytest

import dw_bwd_cases as dc
import dw_fwd_cases as fc
from litehandnet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIN = 16                                                    # LHN_DW_F_FIN
FINALIZE = "lhn_bn_bwd_finalize2 + "
PAIR3, PAIR7 = "k_dw_bwd_data<3> + k_dw_bwd_weight<3,3>", "k_dw_bwd_data<7> + k_dw_bwd_weight<7,1> x 7"


def _table(rows):
    return {case: kern for kern, cases in rows.items() for case in cases.split(", ")}


FWD = _table({
    "k_dwk_fwd_lds<3,1>": "lds3_16, lds3_9x37, lds3_8, lds3_16x33_gate, lds3_c20, lds3_c40, lds3_c80, lds3_notab, fin_lds3",
    "k_dwk_fwd_lds<3,1> ps=2": "par_32, par_17x19, par_3x16, par_16_c40_gate",
    "k_dwk_fwd_lds<3,2>": "d2_8, d2_12x13_c20",
    "k_dwk_fwd_lds<7,1>": "k7_16, k7_9x11_c40_gate",
    "k_dwk_fwd_lds<3,1,2>": "ex_16_so, ex_16, ex_16_fwd2, ex_9x37_c20_so, ex_9x37_c20",
    "k_dwk_fwd_lds<3,1,2> ps=2": "ex_par_17x19_so, ex_par_17x19",
    "k_dws2_fwd_lds": "s2_16, s2_17x19, s2_9_c20_gate, s2_34x66, fin_s2_bias",
    "k_dw_fwd<3>": "g3_4x4, g3_2x2, g3_1x1, g3_7x5_c128, g3_valid, g3_s2d2, g3_c256, g3_c512, g3_c20, g3_c40, fin_g3_4x4",
    "k_dw_fwd<1>": "g1_w, g1_identity",
    "k_dw_fwd<5>": "g5_9",
    "k_dw_fwd<7>": "g7_6x6",
})
FWD_GATHER = _table({
    "k_dw_fwd<3>": "lds3_16, lds3_9x37, lds3_8, lds3_16x33_gate, lds3_c20, lds3_c40, lds3_c80, lds3_notab, par_32, par_17x19, par_3x16, "
                   "par_16_c40_gate, d2_8, d2_12x13_c20, s2_16, s2_17x19, s2_9_c20_gate, s2_34x66",
    "k_dw_fwd<7>": "k7_16, k7_9x11_c40_gate",
})
# the default table of the document is the dispatch without the small-map route (LHN_DW_BWD_SMALL=0) ...
BWD_NOSMALL = _table({
    "k_dw3_bwd_rows<1>": "bench_plain, bench_gy_dpool_acc, bench_xgate_adds_nrep, wide_plain, wide_dpool_adds, small_8, tail_20, tail_80_odd",
    "k_dw3_bwd_rows<1,BNS>": "bench_bns, wide_bns, small_16_bns",
    "k_dw3_bwd_rows<1> ps=2": "parity_32, parity_16_odd, tail_40_parity",
    "k_dw3_bwd_rows<2>": "dil2_narrow_8, dil2_narrow_12",
    "k_dws2_bwd_lds": "s2_16, s2_17x19, s2_9_tail20, s2_34x66",
    "k_dwk_bwd_lds<7,1>": "k7_16, k7_9x21_tail40, k7_12x17_dpool, k7_16_adds",
    PAIR3: "g3_4x4_acc, g3_4x4_dpool, g3_7x5_acc, g3_7x5_dpool, g3_valid, g3_c20, g3_nrep",
    "k_dw_bwd_data<1> + k_dw_bwd_weight<1,1>": "g1_w",
    "k_dw_bwd_data<1>": "g1_identity",
    PAIR7: "g7_6x6",
})
# ... and its small-map section moves four cases (maps of at most 256 pixels) to the FOLD instances of the tile kernel
BWD_SMALL = _table({"k_dwk_bwd_lds<3,1,false,true>": "small_8, tail_20, tail_80_odd", "k_dwk_bwd_lds<3,1,BNS,true>": "small_16_bns"})
BWD = dict(BWD_NOSMALL, **BWD_SMALL)
BWD_V1 = _table({      # the four small-map cases run the FOLD = false instances as before
    "k_dwk_bwd_lds<3,1>": "bench_plain, bench_gy_dpool_acc, bench_xgate_adds_nrep, wide_plain, wide_dpool_adds, small_8, tail_20, tail_80_odd",
    "k_dwk_bwd_lds<3,1,BNS>": "bench_bns, wide_bns, small_16_bns",
    "k_dwk_bwd_lds<3,1> ps=2": "parity_32, parity_16_odd, tail_40_parity",
    "k_dwk_bwd_lds<3,2>": "dil2_narrow_8, dil2_narrow_12",
})
BWD_GATHER = _table({
    PAIR3: "bench_plain, bench_gy_dpool_acc, wide_plain, parity_32, parity_16_odd, dil2_narrow_8, small_8, tail_20, tail_40_parity, s2_16, "
           "s2_17x19, s2_9_tail20, s2_34x66, g3_4x4_acc, g3_4x4_dpool, g3_7x5_acc, g3_7x5_dpool, g3_valid, g3_c20, g3_nrep",
    PAIR7: "k7_16, k7_9x21_tail40, k7_12x17_dpool, g7_6x6",
    "k_dw_bwd_data<1> + k_dw_bwd_weight<1,1>": "g1_w",
    "k_dw_bwd_data<1>": "g1_identity",
    # addends and sums ignore the switch and take the route
    "k_dwk_bwd_lds<3,1,false,true>": "tail_80_odd",
    "k_dwk_bwd_lds<3,1,BNS,true>": "small_16_bns",
})

# n, h, w, cstride, coff, c, dil, flags [, k, stride] of the GPU modules' cases, each run with a finalize source: expected name by
# default (the fold rides in the kernel: no separate launch) and under LHN_DW_BWD_V1=1 (no fold)
WITH_FIN = {
    # tests/test_dw_bwd_small_gpu.py
    "8_bns": ((3, 8, 8, 64, 0, 64, 1, "bns"), "k_dwk_bwd_lds<3,1,BNS,true>", FINALIZE + "k_dwk_bwd_lds<3,1,BNS>"),
    "16_bns": ((2, 16, 16, 64, 0, 64, 1, "bns"), "k_dwk_bwd_lds<3,1,BNS,true>", FINALIZE + "k_dwk_bwd_lds<3,1,BNS>"),
    "32_bns": ((2, 32, 32, 64, 0, 64, 1, "bns"), "k_dw3_bwd_rows<1,BNS>", FINALIZE + "k_dwk_bwd_lds<3,1,BNS>"),
    "9x17_gate_dpool_add": ((2, 9, 17, 64, 0, 64, 1, "ygate dpool add0"), "k_dwk_bwd_lds<3,1,false,true>", FINALIZE + "k_dwk_bwd_lds<3,1>"),
    "8_tail40": ((2, 8, 8, 80, 40, 40, 1, "xgate acc nrep"), "k_dwk_bwd_lds<3,1,false,true>", FINALIZE + "k_dwk_bwd_lds<3,1>"),
    "12_adds": ((2, 12, 12, 32, 0, 32, 1, "add0 add1"), "k_dwk_bwd_lds<3,1,false,true>", FINALIZE + "k_dwk_bwd_lds<3,1>"),
    # tests/test_bwd_fin_consumer_gpu.py
    "c32_16": ((2, 16, 16, 32, 0, 32, 1, ""), "k_dwk_bwd_lds<3,1,false,true>", FINALIZE + "k_dwk_bwd_lds<3,1>"),
    "c64_9x37": ((2, 9, 37, 64, 0, 64, 1, ""), "k_dw3_bwd_rows<1>", FINALIZE + "k_dwk_bwd_lds<3,1>"),
    "c40_8": ((2, 8, 8, 40, 0, 40, 1, ""), "k_dwk_bwd_lds<3,1,false,true>", FINALIZE + "k_dwk_bwd_lds<3,1>"),
    "dil2_17x19": ((2, 17, 19, 64, 0, 64, 2, ""), "k_dw3_bwd_rows<1> ps=2", FINALIZE + "k_dwk_bwd_lds<3,1> ps=2"),
    "dil2_direct_12": ((2, 12, 12, 32, 0, 32, 2, ""), "k_dw3_bwd_rows<2>", FINALIZE + "k_dwk_bwd_lds<3,2>"),
    "bns": ((2, 16, 16, 64, 0, 64, 1, "bns"), "k_dwk_bwd_lds<3,1,BNS,true>", FINALIZE + "k_dwk_bwd_lds<3,1,BNS>"),
    "gate_dpool_adds": ((2, 16, 16, 64, 0, 64, 1, "ygate dpool add0 add1"), "k_dwk_bwd_lds<3,1,false,true>", FINALIZE + "k_dwk_bwd_lds<3,1>"),
    "acc": ((2, 16, 16, 32, 0, 32, 1, "acc"), "k_dwk_bwd_lds<3,1,false,true>", FINALIZE + "k_dwk_bwd_lds<3,1>"),
    "prior_dgamma": ((2, 16, 16, 32, 0, 32, 1, ""), "k_dwk_bwd_lds<3,1,false,true>", FINALIZE + "k_dwk_bwd_lds<3,1>"),
    "slice": ((2, 16, 16, 96, 32, 64, 1, "xgate"), "k_dwk_bwd_lds<3,1,false,true>", FINALIZE + "k_dwk_bwd_lds<3,1>"),
    "s2_launcher": ((2, 16, 16, 32, 0, 32, 1, "", 3, 2), FINALIZE + "k_dws2_bwd_lds", FINALIZE + "k_dws2_bwd_lds"),
    "gather_launcher": ((2, 4, 4, 64, 0, 64, 1, "acc"), FINALIZE + PAIR3, FINALIZE + PAIR3),
    # K = 7 never folds
    "k7_16": ((2, 16, 16, 32, 0, 32, 1, "", 7), FINALIZE + "k_dwk_bwd_lds<7,1>", FINALIZE + "k_dwk_bwd_lds<7,1>"),
}


def test_forward_tables():
    assert set(FWD) == set(fc.CASES)
    for nm, want in FWD.items():
        assert fc.kernel_of(nm) == want, nm
    for nm, want in FWD_GATHER.items():
        assert fc.kernel_of(nm, gather=True) == want, nm


def test_backward_tables():
    assert set(BWD) == set(dc.CASES)
    for nm, want in BWD.items():
        assert dc.kernel_of(nm) == want, nm
        assert dc.kernel_of(nm, small=False) == BWD_NOSMALL[nm], nm
    for nm, want in BWD_V1.items():
        assert dc.kernel_of(nm, v1=True) == want, nm
    for nm, want in BWD_GATHER.items():
        assert dc.kernel_of(nm, gather=True) == want, nm


@pytest.mark.parametrize("case", sorted(WITH_FIN))
def test_backward_with_finalize_source(case):
    tup, want, want_v1 = WITH_FIN[case]
    n, h, w, cs, coff, c, dil, flags, k, stride, pad = dc._case(*tup)
    f = flags.split()
    feat = FIN | dc.F_BNSUM * ("bns" in f) | dc.F_ADDS * ("add0" in f or "add1" in f) | dc.F_DX_ACC * ("acc" in f)
    route = lambda sw: _lib.lib().lhn_conv_dw_route(1, h, w, c, k, stride, pad, dil, feat, sw).decode()      # noqa: E731
    assert route(dc.SW_BWD_SMALL) == want
    assert route(dc.SW_BWD_SMALL | dc.SW_BWD_V1) == want_v1


def test_no_kernel_is_null():
    for nm in ("bns_k7", "bns_dil2"):
        assert dc.kernel_of(nm) is None, nm
    for nm in ("extra_k7", "extra_w4", "extra_d2_w12"):
        assert fc.kernel_of(nm) is None, nm


def test_environment_is_read():
    """switches = -1: as the process read them.  Here nothing is set; a child sets LHN_DW_GATHER=1."""
    ask = ("import sys; sys.path.insert(0, %r); from litehandnet_amd import _lib; L = _lib.lib(); "
           "print(L.lhn_conv_dw_route(0, 16, 16, 64, 3, 1, 1, 1, 0, -1).decode()); "
           "print(L.lhn_conv_dw_route(1, 64, 64, 64, 3, 1, 1, 1, 0, -1).decode()); "
           "print(L.lhn_conv_dw_route(1, 64, 64, 64, 3, 1, 1, 1, 4, -1).decode())" % ROOT)
    env = {k: v for k, v in os.environ.items() if not k.startswith("LHN_DW_")}
    plain = subprocess.run([sys.executable, "-c", ask], env=env, capture_output=True, text=True, check=True).stdout.split("\n")[:3]
    assert plain == ["k_dwk_fwd_lds<3,1>", "k_dw3_bwd_rows<1>", "k_dw3_bwd_rows<1,BNS>"]
    child = subprocess.run([sys.executable, "-c", ask], env=dict(env, LHN_DW_GATHER="1"), capture_output=True, text=True, check=True)
    assert child.stdout.split("\n")[:3] == ["k_dw_fwd<3>", PAIR3, "k_dw3_bwd_rows<1,BNS>"]
