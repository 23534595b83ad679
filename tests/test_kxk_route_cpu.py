"""CPU: the dense 3x3 route (lhn_conv_kxk_route: host only, the functions lhn_conv_kxk_fwd / lhn_conv_kxk_bwd themselves ask) against a
literal table written down from the dispatch code as it stood before the route existed (its arithmetic, and the case-to-kernel tables
the docstrings of kxk_cases.py / kxk256_cases.py carried): every case of FWD / BWD of both case modules on 256 CUs, on 2 CUs with 16
gradient replicas (the LHN_DETERMINISTIC=1 child), under LHN_PLAIN=0 and LHN_PLAIN=1; the refusals; the thresholds of the tile rules;
the harness's plain_path() against the answer; one child process that sets LHN_PLAIN=0.
Spelling (include/lhn.h): " yN" blocks of features on gridDim.y, " par" the parity classes of the stride-2 data gradient, " zN" groups
of output channels on gridDim.z, " excl" / " atomic" the weight gradient's flush, " x 2" one launch per 128-channel input slice."""
import os
import subprocess
import sys

import kxk256_cases as k2
import kxk_cases as kc
from litehandnet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DY, WT = "k_dy_inplace + ", "k_w_tapmajor + "


def _table(rows):
    return {case: kern for kern, cases in rows.items() for case in cases.split(", ")}


# ---------------------------------------------------------------- forward: k_w_tapmajor, k_kxk<Cin, NT, 0, 9, false>
FWD = _table({
    WT + "k_kxk<32, 1, 0, 9, false>": "pair_32_32, s2_32_32_odd, s2_32_32_even, mt_32_32, big_32_32",
    WT + "k_kxk<32, 1, 0, 9, false> y2": "pair_32_64, tail_32_48, mt_32_64",
    WT + "k_kxk<32, 1, 0, 9, false> y4": "pair_32_128, tiny_32_128, mt_32_128",
    WT + "k_kxk<32, 1, 0, 9, false> y8": "pair_32_256",
    WT + "k_kxk<64, 1, 0, 9, false>": "pair_64_32, mt_64_32",
    WT + "k_kxk<64, 1, 0, 9, false> y2": "pair_64_64, tiny_64_64, view_64_64, s2_64_64_odd, s2_64_64_even, nostats_64_64, tail_64_40, mt_64_64",
    WT + "k_kxk<64, 1, 0, 9, false> y4": "pair_64_128, mt_64_128",
    WT + "k_kxk<64, 1, 0, 9, false> y8": "pair_64_256, mt_64_256",
    WT + "k_kxk<128, 1, 0, 9, false>": "pair_128_32, view_128_32, mt_128_32",
    WT + "k_kxk<128, 1, 0, 9, false> y2": "pair_128_64, s2_128_64_odd, s2_128_64_even, tail_128_40, mt_128_64",
    WT + "k_kxk<128, 1, 0, 9, false> y4": "pair_128_128, mt_128_128",
    WT + "k_kxk<128, 1, 0, 9, false> y8": "pair_128_256, mt_128_256",
    WT + "k_kxk<128, 4, 0, 9, false>": "big_128_128",                              # 517 tiles: no split
    WT + "k_kxk<256, 1, 0, 9, false>": "pair_256_32",
    WT + "k_kxk<256, 1, 0, 9, false> y2": "pair_256_64, tail_256_40, mt_256_64",
    WT + "k_kxk<256, 1, 0, 9, false> y4": "pair_256_128, mt_256_128",
    WT + "k_kxk<256, 1, 0, 9, false> y8": "pair_256_256, tiny_256_256, view_256_256, s2_256_256_odd, s2_256_256_even, mt_256_256",
    WT + "k_kxk<256, 4, 0, 9, false> y2": "big_256_256",                           # 292 tiles: 256 features start from two splits
})
FWD_DET = _table({        # 2 CUs: splitting stops at 4 workgroups
    WT + "k_kxk<32, 2, 0, 9, false>": "mt_32_64",
    WT + "k_kxk<32, 2, 0, 9, false> y2": "pair_32_128",
    WT + "k_kxk<32, 4, 0, 9, false>": "mt_32_128",
    WT + "k_kxk<32, 4, 0, 9, false> y2": "pair_32_256",
    WT + "k_kxk<64, 2, 0, 9, false>": "view_64_64, mt_64_64",
    WT + "k_kxk<64, 2, 0, 9, false> y2": "pair_64_128",
    WT + "k_kxk<64, 4, 0, 9, false>": "mt_64_128",
    WT + "k_kxk<64, 4, 0, 9, false> y2": "pair_64_256, mt_64_256",
    WT + "k_kxk<128, 2, 0, 9, false>": "mt_128_64",
    WT + "k_kxk<128, 2, 0, 9, false> y2": "pair_128_128",
    WT + "k_kxk<128, 4, 0, 9, false>": "mt_128_128",
    WT + "k_kxk<128, 4, 0, 9, false> y2": "pair_128_256, mt_128_256",
    WT + "k_kxk<256, 2, 0, 9, false>": "mt_256_64",
    WT + "k_kxk<256, 2, 0, 9, false> y2": "pair_256_128",
    WT + "k_kxk<256, 2, 0, 9, false> y4": "tiny_256_256, s2_256_256_odd, s2_256_256_even",
    WT + "k_kxk<256, 4, 0, 9, false>": "mt_256_128",
    WT + "k_kxk<256, 4, 0, 9, false> y2": "pair_256_256, view_256_256, mt_256_256",
})

# ---------------------------------------------------------------- backward: k_dy_inplace, k_w_tapmajor, k_kxk<Cout, NT, 1, 9, PLAIN>,
# k_kxk_wgrad<min(Cin, 128), NTO, 9, PLAIN>
BWD = _table({
    WT + "k_kxk<32, 1, 1, 9, false> + k_kxk_wgrad<32, 1, 9, false> atomic": "pair_32_32, rep1_32_32, mt_32_32",
    WT + "k_kxk<64, 1, 1, 9, false> + k_kxk_wgrad<32, 2, 9, false> atomic": "pair_32_64, rep1_32_64, fly_32_64, mt_32_64",
    DY + WT + "k_kxk<128, 1, 1, 9, true> + k_kxk_wgrad<32, 4, 9, true> atomic": "pair_32_128, rep1_32_128, full_32_128, mt_32_128",
    WT + "k_kxk<32, 1, 1, 9, false> y2 + k_kxk_wgrad<64, 1, 9, false> atomic": "pair_64_32, rep1_64_32, fly_64_32, mt_64_32",
    DY + WT + "k_kxk<64, 1, 1, 9, true> y2 + k_kxk_wgrad<64, 1, 9, true> z2 excl": "pair_64_64, cosplit_64_64, full_64_64, xgate_64_64, mt_64_64",
    DY + WT + "k_kxk<128, 1, 1, 9, true> y2 + k_kxk_wgrad<64, 1, 9, true> z4 excl": "pair_64_128, cosplit_64_128, mt_64_128",
    DY + WT + "k_kxk<32, 1, 1, 9, true> y4 + k_kxk_wgrad<128, 1, 9, true> atomic": "pair_128_32, rep1_128_32, mt_128_32",
    DY + WT + "k_kxk<64, 1, 1, 9, true> y4 + k_kxk_wgrad<128, 1, 9, true> z2 excl": "pair_128_64, cosplit_128_64, mt_128_64",
    DY + WT + "k_kxk<128, 1, 1, 9, true> y4 + k_kxk_wgrad<128, 1, 9, true> z4 excl": "pair_128_128, cosplit_128_128, mt_128_128",
    DY + WT + "k_kxk<64, 1, 1, 9, true> y2 + k_kxk_wgrad<64, 2, 9, true> atomic": "rep1_64_64, nocosplit_64_64",      # one replica; 66 tiles
    DY + WT + "k_kxk<128, 1, 1, 9, true> y2 + k_kxk_wgrad<64, 4, 9, true> atomic": "rep1_64_128",
    DY + WT + "k_kxk<64, 1, 1, 9, true> y4 + k_kxk_wgrad<128, 2, 9, true> atomic": "rep1_128_64",
    DY + WT + "k_kxk<128, 1, 1, 9, true> y4 + k_kxk_wgrad<128, 4, 9, true> atomic": "rep1_128_128",
    DY + WT + "k_kxk<32, 1, 1, 9, true> + k_kxk_wgrad<32, 1, 9, true> atomic": "dpool_32_32",                          # a pooled gradient below 4096
    DY + "k_kxk_wgrad<64, 1, 9, true> z2 excl": "nodx_64_64",
    DY + "k_kxk_wgrad<128, 1, 9, true> z4 excl": "nodx_128_128",
    DY + WT + "k_kxk<64, 1, 1, 9, true> y4 par + k_kxk_wgrad<128, 1, 9, true> z2 excl":
        "s2_128_64_odd_store, s2_128_64_odd_acc, s2_128_64_even_store, s2_128_64_even_acc",
    WT + "k_kxk<32, 1, 1, 9, false> par + k_kxk_wgrad<32, 1, 9, false> excl":
        "s2_32_32_odd_store, s2_32_32_odd_acc, s2_32_32_even_store, s2_32_32_even_acc",
    DY + WT + "k_kxk<128, 4, 1, 9, true> + k_kxk_wgrad<128, 4, 9, true> atomic": "big_128_128",
    # a side of 256 (kxk256_cases)
    DY + WT + "k_kxk<256, 1, 1, 9, true> y8 + k_kxk_wgrad<128, 1, 9, true> z8 excl x 2":
        "pair_256_256, tiny_256_256, mt_256_256, cosplit_256_256, full_256_256",
    DY + WT + "k_kxk<128, 1, 1, 9, true> y8 + k_kxk_wgrad<128, 1, 9, true> z4 excl x 2": "pair_256_128, mt_256_128",
    DY + WT + "k_kxk<64, 1, 1, 9, true> y8 + k_kxk_wgrad<128, 1, 9, true> z2 excl x 2": "pair_256_64, mt_256_64",
    DY + WT + "k_kxk<32, 1, 1, 9, true> y8 + k_kxk_wgrad<128, 1, 9, true> atomic x 2": "pair_256_32, rep1_256_32",
    DY + WT + "k_kxk<256, 1, 1, 9, true> y4 + k_kxk_wgrad<128, 1, 9, true> z8 excl": "pair_128_256, mt_128_256",
    DY + WT + "k_kxk<256, 1, 1, 9, true> y2 + k_kxk_wgrad<64, 1, 9, true> z8 excl": "pair_64_256, mt_64_256",
    DY + WT + "k_kxk<256, 1, 1, 9, true> + k_kxk_wgrad<32, 4, 9, true> z2 atomic": "pair_32_256, rep1_32_256",        # Cin = 32: never chunked
    DY + WT + "k_kxk<256, 1, 1, 9, true> y8 + k_kxk_wgrad<128, 4, 9, true> z2 atomic x 2": "rep1_256_256, nocosplit_256_256",
    DY + WT + "k_kxk<128, 1, 1, 9, true> y8 + k_kxk_wgrad<128, 4, 9, true> atomic x 2": "rep1_256_128",
    DY + WT + "k_kxk<64, 1, 1, 9, true> y8 + k_kxk_wgrad<128, 2, 9, true> atomic x 2": "rep1_256_64",
    DY + WT + "k_kxk<256, 1, 1, 9, true> y4 + k_kxk_wgrad<128, 4, 9, true> z2 atomic": "rep1_128_256",
    DY + WT + "k_kxk<256, 1, 1, 9, true> y2 + k_kxk_wgrad<64, 4, 9, true> z2 atomic": "rep1_64_256",
    DY + WT + "k_kxk<256, 1, 1, 9, true> y8 par + k_kxk_wgrad<128, 1, 9, true> z8 excl x 2":
        "s2_256_256_odd_store, s2_256_256_odd_acc, s2_256_256_even_store, s2_256_256_even_acc",
    DY + "k_kxk_wgrad<128, 1, 9, true> z8 excl x 2": "nodx_256_256",
    DY + WT + "k_kxk<256, 4, 1, 9, true> y2 + k_kxk_wgrad<128, 4, 9, true> z2 atomic x 2": "big_256_256",
})
BWD_DET = _table({        # 2 CUs, 16 replicas: every flush exclusive, every case with Cin >= 64 chunked
    WT + "k_kxk<32, 1, 1, 9, false> + k_kxk_wgrad<32, 1, 9, false> excl": "pair_32_32, rep1_32_32, mt_32_32",
    WT + "k_kxk<64, 1, 1, 9, false> + k_kxk_wgrad<32, 2, 9, false> excl": "pair_32_64, rep1_32_64, fly_32_64, mt_32_64",
    DY + WT + "k_kxk<128, 1, 1, 9, true> + k_kxk_wgrad<32, 4, 9, true> excl": "pair_32_128, rep1_32_128, full_32_128, mt_32_128",
    WT + "k_kxk<32, 1, 1, 9, false> y2 + k_kxk_wgrad<64, 1, 9, false> excl": "pair_64_32, rep1_64_32",
    WT + "k_kxk<32, 2, 1, 9, false> + k_kxk_wgrad<64, 1, 9, false> excl": "fly_64_32, mt_64_32",
    DY + WT + "k_kxk<64, 1, 1, 9, true> y2 + k_kxk_wgrad<64, 1, 9, true> z2 excl": "rep1_64_64",
    DY + WT + "k_kxk<128, 1, 1, 9, true> y2 + k_kxk_wgrad<64, 1, 9, true> z4 excl": "rep1_64_128",
    DY + WT + "k_kxk<64, 2, 1, 9, true> + k_kxk_wgrad<64, 1, 9, true> z2 excl": "cosplit_64_64, nocosplit_64_64, full_64_64, mt_64_64",
    DY + WT + "k_kxk<128, 2, 1, 9, true> + k_kxk_wgrad<64, 1, 9, true> z4 excl": "cosplit_64_128, mt_64_128",
    DY + WT + "k_kxk<32, 2, 1, 9, true> y2 + k_kxk_wgrad<128, 1, 9, true> excl": "pair_128_32, rep1_128_32",
    DY + WT + "k_kxk<64, 2, 1, 9, true> y2 + k_kxk_wgrad<128, 1, 9, true> z2 excl": "pair_128_64, rep1_128_64",
    DY + WT + "k_kxk<128, 2, 1, 9, true> y2 + k_kxk_wgrad<128, 1, 9, true> z4 excl": "pair_128_128, rep1_128_128",
    DY + WT + "k_kxk<32, 4, 1, 9, true> + k_kxk_wgrad<128, 1, 9, true> excl": "mt_128_32",
    DY + WT + "k_kxk<64, 4, 1, 9, true> + k_kxk_wgrad<128, 1, 9, true> z2 excl": "cosplit_128_64, mt_128_64",
    DY + WT + "k_kxk<128, 4, 1, 9, true> + k_kxk_wgrad<128, 1, 9, true> z4 excl": "cosplit_128_128, mt_128_128",
    DY + WT + "k_kxk<32, 1, 1, 9, true> + k_kxk_wgrad<32, 1, 9, true> excl": "dpool_32_32",
    DY + WT + "k_kxk<64, 2, 1, 9, true> y2 par + k_kxk_wgrad<128, 1, 9, true> z2 excl": "s2_128_64_odd_store, s2_128_64_odd_acc",
    DY + WT + "k_kxk<128, 4, 1, 9, true> + k_kxk_wgrad<128, 4, 9, true> excl": "big_128_128",      # 1,033 tiles > 16 * 16: not chunked
    DY + WT + "k_kxk<256, 4, 1, 9, true> y2 + k_kxk_wgrad<128, 1, 9, true> z8 excl x 2":
        "pair_256_256, rep1_256_256, mt_256_256, cosplit_256_256, nocosplit_256_256, full_256_256",
    DY + WT + "k_kxk<128, 4, 1, 9, true> y2 + k_kxk_wgrad<128, 1, 9, true> z4 excl x 2": "pair_256_128, rep1_256_128, mt_256_128",
    DY + WT + "k_kxk<64, 4, 1, 9, true> y2 + k_kxk_wgrad<128, 1, 9, true> z2 excl x 2": "pair_256_64, rep1_256_64, mt_256_64",
    DY + WT + "k_kxk<32, 4, 1, 9, true> y2 + k_kxk_wgrad<128, 1, 9, true> excl x 2": "pair_256_32, rep1_256_32",
    DY + WT + "k_kxk<256, 2, 1, 9, true> y2 + k_kxk_wgrad<128, 1, 9, true> z8 excl": "pair_128_256, rep1_128_256",
    DY + WT + "k_kxk<256, 4, 1, 9, true> + k_kxk_wgrad<128, 1, 9, true> z8 excl": "mt_128_256",
    DY + WT + "k_kxk<256, 1, 1, 9, true> y2 + k_kxk_wgrad<64, 1, 9, true> z8 excl": "rep1_64_256",
    DY + WT + "k_kxk<256, 2, 1, 9, true> + k_kxk_wgrad<64, 1, 9, true> z8 excl": "mt_64_256",
    DY + WT + "k_kxk<256, 1, 1, 9, true> + k_kxk_wgrad<32, 4, 9, true> z2 excl": "pair_32_256, rep1_32_256",
    DY + WT + "k_kxk<256, 2, 1, 9, true> y4 + k_kxk_wgrad<128, 1, 9, true> z8 excl x 2": "tiny_256_256",
    DY + WT + "k_kxk<256, 4, 1, 9, true> y2 par + k_kxk_wgrad<128, 1, 9, true> z8 excl x 2": "s2_256_256_odd_store, s2_256_256_odd_acc",
    DY + WT + "k_kxk<256, 2, 1, 9, true> y4 par + k_kxk_wgrad<128, 1, 9, true> z8 excl x 2": "s2_256_256_even_store, s2_256_256_even_acc",
    DY + WT + "k_kxk<256, 4, 1, 9, true> y2 + k_kxk_wgrad<128, 4, 9, true> z2 excl x 2": "big_256_256",
})
BWD_PLAIN0 = _table({     # dy on the fly wherever the size rule alone made the call plain; a pooled gradient or a side of 256 stays
    WT + "k_kxk<128, 1, 1, 9, false> + k_kxk_wgrad<32, 4, 9, false> atomic": "pair_32_128, rep1_32_128, mt_32_128",
    WT + "k_kxk<64, 1, 1, 9, false> y2 + k_kxk_wgrad<64, 1, 9, false> z2 excl": "pair_64_64, cosplit_64_64, xgate_64_64, mt_64_64",
    WT + "k_kxk<128, 1, 1, 9, false> y2 + k_kxk_wgrad<64, 1, 9, false> z4 excl": "pair_64_128, cosplit_64_128, mt_64_128",
    WT + "k_kxk<32, 1, 1, 9, false> y4 + k_kxk_wgrad<128, 1, 9, false> atomic": "pair_128_32, rep1_128_32, mt_128_32",
    WT + "k_kxk<64, 1, 1, 9, false> y4 + k_kxk_wgrad<128, 1, 9, false> z2 excl": "pair_128_64, cosplit_128_64, mt_128_64",
    WT + "k_kxk<128, 1, 1, 9, false> y4 + k_kxk_wgrad<128, 1, 9, false> z4 excl": "pair_128_128, cosplit_128_128, mt_128_128",
    WT + "k_kxk<64, 1, 1, 9, false> y2 + k_kxk_wgrad<64, 2, 9, false> atomic": "rep1_64_64, nocosplit_64_64",
    WT + "k_kxk<128, 1, 1, 9, false> y2 + k_kxk_wgrad<64, 4, 9, false> atomic": "rep1_64_128",
    WT + "k_kxk<64, 1, 1, 9, false> y4 + k_kxk_wgrad<128, 2, 9, false> atomic": "rep1_128_64",
    WT + "k_kxk<128, 1, 1, 9, false> y4 + k_kxk_wgrad<128, 4, 9, false> atomic": "rep1_128_128",
    "k_kxk_wgrad<64, 1, 9, false> z2 excl": "nodx_64_64",
    "k_kxk_wgrad<128, 1, 9, false> z4 excl": "nodx_128_128",
    WT + "k_kxk<64, 1, 1, 9, false> y4 par + k_kxk_wgrad<128, 1, 9, false> z2 excl":
        "s2_128_64_odd_store, s2_128_64_odd_acc, s2_128_64_even_store, s2_128_64_even_acc",
    WT + "k_kxk<128, 4, 1, 9, false> + k_kxk_wgrad<128, 4, 9, false> atomic": "big_128_128",
})
BWD_PLAIN1 = _table({     # the four pairs below 4096 without a pooled gradient
    DY + WT + "k_kxk<32, 1, 1, 9, true> + k_kxk_wgrad<32, 1, 9, true> atomic": "pair_32_32, rep1_32_32, mt_32_32",
    DY + WT + "k_kxk<64, 1, 1, 9, true> + k_kxk_wgrad<32, 2, 9, true> atomic": "pair_32_64, rep1_32_64, fly_32_64, mt_32_64",
    DY + WT + "k_kxk<32, 1, 1, 9, true> y2 + k_kxk_wgrad<64, 1, 9, true> atomic": "pair_64_32, rep1_64_32, fly_64_32, mt_64_32",
    DY + WT + "k_kxk<32, 1, 1, 9, true> par + k_kxk_wgrad<32, 1, 9, true> excl":
        "s2_32_32_odd_store, s2_32_32_odd_acc, s2_32_32_even_store, s2_32_32_even_acc",
})
SETTINGS = {"default": {}, "det": {"cus": 2}, "plain0": {"plain": 0}, "plain1": {"plain": 1}}
SWITCHED = {"fwd": {"det": FWD_DET, "plain0": {}, "plain1": {}}, "bwd": {"det": BWD_DET, "plain0": BWD_PLAIN0, "plain1": BWD_PLAIN1}}


def _ask(backward, nhw, cin, cout, stride=1, nrep=4, feat=kc.F_DX, cus=256, sw=0):
    r = _lib.lib().lhn_conv_kxk_route(backward, nhw[0], nhw[1], nhw[2], cin, cout, stride, nrep, feat, cus, sw)
    return r.decode() if r is not None else None


def test_forward_tables():
    assert set(FWD) == set(kc.FWD) | set(k2.FWD)
    for nm, want in FWD.items():
        assert kc.kernel_of("fwd", nm) == want, nm
        assert kc.kernel_of("fwd", nm, wt=False) == want[len(WT):], nm
        for tag, kw in SETTINGS.items():
            assert kc.kernel_of("fwd", nm, **kw) == SWITCHED["fwd"].get(tag, {}).get(nm, want), (nm, tag)


def test_backward_tables():
    assert set(BWD) == set(kc.BWD) | set(k2.BWD)
    for nm, want in BWD.items():
        assert kc.kernel_of("bwd", nm) == want, nm
        assert kc.kernel_of("bwd", nm, wt=False) == want.replace(WT, ""), nm
        for tag, kw in SETTINGS.items():
            assert kc.kernel_of("bwd", nm, **kw) == SWITCHED["bwd"].get(tag, {}).get(nm, want), (nm, tag)


def test_switched_tables_name_only_cases_that_change():
    for kind, base in (("fwd", FWD), ("bwd", BWD)):
        for tag, tab in SWITCHED[kind].items():
            for nm, want in tab.items():
                assert want != base[nm], (kind, tag, nm)


def test_refusals_are_null():
    """Every refused case, under every setting -- but fwd:r_geometry, whose channels have a kernel: its y is one row too tall, and
    the query is not told y's geometry (the call itself checks it first)."""
    for kind, tabs in (("fwd", (kc.FWD_REFUSE, k2.FWD_REFUSE)), ("bwd", (kc.BWD_REFUSE, k2.BWD_REFUSE))):
        for tab in tabs:
            for nm, c in tab.items():
                for tag, kw in SETTINGS.items():
                    got = kc.kernel_of(kind, nm, **kw)
                    if "badgeo" in c["flags"]:
                        assert (kind, nm) == ("fwd", "r_geometry") and got == WT + "k_kxk<64, 1, 0, 9, false> y2", (kind, nm, tag)
                    else:
                        assert got is None, (kind, nm, tag)
    for stride in (0, 3, -1):
        assert _ask(0, (2, 9, 9), 64, 64, stride) is None and _ask(1, (2, 9, 9), 64, 64, stride) is None


def test_feature_split_thresholds():
    """kxk_nt_block: split the feature tiles while tiles * splits < 2 * cus.  Tiles of 128 pixels; W = 128, so H counts them."""
    fwd = lambda tiles, cout, cus=256, cin=64: _ask(0, (1, tiles, 128), cin, cout, feat=0, cus=cus)      # noqa: E731
    assert fwd(511, 64) == "k_kxk<64, 1, 0, 9, false> y2"            # 511 < 512: split
    assert fwd(512, 64) == "k_kxk<64, 2, 0, 9, false>"
    assert fwd(255, 128) == "k_kxk<64, 1, 0, 9, false> y4"           # 255 * 2 < 512: a second split
    assert fwd(256, 128) == "k_kxk<64, 2, 0, 9, false> y2"
    # eight feature tiles start from two splits, whatever the map
    assert fwd(127, 256) == "k_kxk<64, 1, 0, 9, false> y8"
    assert fwd(128, 256) == "k_kxk<64, 2, 0, 9, false> y4"
    assert fwd(255, 256) == "k_kxk<64, 2, 0, 9, false> y4"
    assert fwd(512, 256) == fwd(100000, 256) == "k_kxk<64, 4, 0, 9, false> y2"
    assert fwd(1, 256, cus=2) == "k_kxk<64, 2, 0, 9, false> y4"      # 1 * 2 < 4
    assert fwd(3, 256, cus=2) == fwd(4, 256, cus=2) == "k_kxk<64, 4, 0, 9, false> y2"
    assert fwd(127, 256, cus=2, cin=256) == "k_kxk<256, 4, 0, 9, false> y2"
    # the data gradient splits Cin's tiles by x's pixels the same way
    bwd = lambda tiles, cin: _ask(1, (1, tiles, 128), cin, 64, nrep=1).split(" + ")[1]      # noqa: E731
    assert bwd(511, 64) == "k_kxk<64, 1, 1, 9, true> y2" and bwd(512, 64) == "k_kxk<64, 2, 1, 9, true>"
    assert bwd(512, 256) == "k_kxk<64, 4, 1, 9, true> y2"


def test_weight_gradient_thresholds():
    """chunked (pixel chunks = replicas, one 32-channel group per block): Cin >= 64, nrep > 1, at most 16 * nrep tiles of 64 pixels."""
    wg = lambda nhw, cin, cout, nrep=4, **kw: _ask(1, nhw, cin, cout, nrep=nrep, **kw).split(" + ")[-1]      # noqa: E731
    assert wg((1, 64, 64), 64, 64) == "k_kxk_wgrad<64, 1, 9, true> z2 excl"              # 64 tiles = 16 * 4
    assert wg((1, 64, 65), 64, 64) == "k_kxk_wgrad<64, 2, 9, true> atomic"               # 65
    assert wg((1, 66, 64), 64, 64) == "k_kxk_wgrad<64, 2, 9, true> atomic"               # 66
    assert wg((1, 64, 64), 256, 256) == "k_kxk_wgrad<128, 1, 9, true> z8 excl x 2"
    assert wg((1, 64, 65), 256, 256) == "k_kxk_wgrad<128, 4, 9, true> z2 atomic x 2"     # 256 features: two groups of four tiles
    for nhw in ((1, 64, 64), (1, 64, 65), (2, 8, 8)):                                    # one replica: never chunked
        assert wg(nhw, 64, 64, nrep=1) == "k_kxk_wgrad<64, 2, 9, true> atomic"
    assert wg((1, 8, 8), 64, 64, nrep=1) == "k_kxk_wgrad<64, 2, 9, true> excl"           # one tile, one block: it owns the replica
    assert wg((2, 8, 8), 32, 64) == "k_kxk_wgrad<32, 2, 9, false> excl"                  # Cin = 32: never chunked
    assert wg((2, 8, 8), 32, 256) == "k_kxk_wgrad<32, 4, 9, true> z2 excl"
    assert wg((1, 64, 64), 64, 64, cus=2, nrep=16) == "k_kxk_wgrad<64, 1, 9, true> z2 excl"


def test_plain_rule():
    dy = lambda cin, cout, feat=kc.F_DX, sw=0: _ask(1, (2, 8, 8), cin, cout, feat=feat, sw=sw).startswith("k_dy_inplace")      # noqa: E731
    # Cin * Cout on both sides of 4096 with the switch unset
    assert not dy(32, 64) and not dy(64, 32) and dy(32, 128) and dy(128, 32) and dy(64, 64)
    assert _ask(1, (2, 8, 8), 32, 64) == "k_kxk<64, 1, 1, 9, false> + k_kxk_wgrad<32, 2, 9, false> excl"
    assert _ask(1, (2, 8, 8), 32, 128) == "k_dy_inplace + k_kxk<128, 1, 1, 9, true> + k_kxk_wgrad<32, 4, 9, true> excl"
    # the switch replaces the size rule ...
    assert not dy(128, 128, sw=kc.SW_PLAIN0) and dy(32, 32, sw=kc.SW_PLAIN1) and not dy(32, 32)
    # ... and nothing else: a pooled gradient below 4096, a side of 256
    assert dy(32, 32, kc.F_DX | kc.F_DPOOL) and dy(32, 32, kc.F_DX | kc.F_DPOOL, kc.SW_PLAIN0)
    assert _ask(1, (2, 8, 8), 256, 32, sw=kc.SW_PLAIN0) == "k_dy_inplace + k_kxk<32, 1, 1, 9, true> y8 + k_kxk_wgrad<128, 1, 9, true> excl x 2"
    assert _ask(1, (2, 8, 8), 32, 256, sw=kc.SW_PLAIN0) == "k_dy_inplace + k_kxk<256, 1, 1, 9, true> + k_kxk_wgrad<32, 4, 9, true> z2 excl"


def test_no_dx_and_stride2():
    # dx NULL: no data gradient, no weight re-lay, and no data-gradient instance is required to exist (K = Cout = 40 has none)
    assert _ask(1, (2, 8, 8), 64, 40, feat=kc.F_WT) == "k_kxk_wgrad<64, 1, 9, false> z2 excl"
    assert _ask(1, (2, 8, 8), 64, 40, feat=kc.F_DX | kc.F_WT) is None
    assert _ask(1, (2, 9, 9), 64, 64, 2, feat=kc.F_WT) == "k_dy_inplace + k_kxk_wgrad<64, 1, 9, true> z2 excl"
    # stride 2: four parity classes of input pixels
    assert _ask(1, (2, 9, 9), 64, 64, 2, feat=kc.F_DX | kc.F_WT) == \
        "k_dy_inplace + k_w_tapmajor + k_kxk<64, 1, 1, 9, true> y2 par + k_kxk_wgrad<64, 1, 9, true> z2 excl"
    assert _ask(0, (2, 9, 9), 64, 64, 2, feat=kc.F_WT) == "k_w_tapmajor + k_kxk<64, 1, 0, 9, false> y2"


def test_plain_path_is_the_routes_answer(monkeypatch):
    """The harness's own statement of the rule (kxk_cases.plain_path reads the environment) against the library's, for every backward
    case under every setting: the two cannot drift apart silently."""
    for tag, kw in SETTINGS.items():
        if "plain" in kw:
            monkeypatch.setenv("LHN_PLAIN", str(kw["plain"]))
        else:
            monkeypatch.delenv("LHN_PLAIN", raising=False)
        for nm in BWD:
            assert kc.plain_path(kc._ALL["bwd"][nm]) == ("k_dy_inplace" in kc.kernel_of("bwd", nm, **kw)), (nm, tag)
    monkeypatch.setenv("LHN_PLAIN", "")          # set but empty: set, and not '1'
    for nm in BWD:
        assert kc.plain_path(kc._ALL["bwd"][nm]) == ("k_dy_inplace" in kc.kernel_of("bwd", nm, plain=0)), nm


def test_environment_is_read():
    """switches = -1: as the process read LHN_PLAIN, once.  Here a child without it, and one that sets LHN_PLAIN=0."""
    ask = ("import sys; sys.path.insert(0, %r); from litehandnet_amd import _lib; L = _lib.lib(); "
           "print(L.lhn_conv_kxk_route(1, 2, 8, 8, 64, 64, 1, 4, 1, 256, -1).decode()); "
           "print(L.lhn_conv_kxk_route(1, 2, 8, 8, 256, 64, 1, 4, 1, 256, -1).decode())" % ROOT)
    env = {k: v for k, v in os.environ.items() if k not in ("LHN_PLAIN", "LHN_DETERMINISTIC")}
    unset = subprocess.run([sys.executable, "-c", ask], env=env, capture_output=True, text=True, check=True).stdout.split("\n")[:2]
    assert unset == ["k_dy_inplace + k_kxk<64, 1, 1, 9, true> y2 + k_kxk_wgrad<64, 1, 9, true> z2 excl",
                     "k_dy_inplace + k_kxk<64, 1, 1, 9, true> y8 + k_kxk_wgrad<128, 1, 9, true> z2 excl x 2"]
    child = subprocess.run([sys.executable, "-c", ask], env=dict(env, LHN_PLAIN="0"), capture_output=True, text=True, check=True)
    assert child.stdout.split("\n")[:2] == ["k_kxk<64, 1, 1, 9, false> y2 + k_kxk_wgrad<64, 1, 9, false> z2 excl", unset[1]]
