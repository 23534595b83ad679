"""CPU: the dense 3x3 route (lhn_conv_kxk_route: host only, what lhn_conv_kxk_fwd / lhn_conv_kxk_bwd themselves ask) at 40 and 160
channels.  For every case of tests/kxk160_cases.py and each of the four settings of profiles/kxk160_instances.md the library names
its launches, the instance names follow the rules the case file states (K = Cin forward, K = Cout in the data gradient; 160 -> NT 5 or
gridDim.y = 5; the weight gradient of a 160-channel input as a 128- and a 32-channel launch), and the harness's plain_path() equals
what the route answers.  The mixed pairs, and every older refusal that a test pins, give no route.  On a library without the
width-160 instances every case of the tables answers NULL."""
import os
import re

import pytest

import kxk160_cases as k6
import kxk_cases as kc

DY = "k_dy_inplace + "
CASES = [(kind, nm) for kind, t in k6.TABLES.items() for nm in t]


def _plain_under(c, plain):
    """kxk_cases.plain_path under a setting's LHN_PLAIN (None: unset) instead of this process's."""
    old = os.environ.pop("LHN_PLAIN", None)
    try:
        if plain is not None:
            os.environ["LHN_PLAIN"] = str(plain)
        return kc.plain_path(c)
    finally:
        os.environ.pop("LHN_PLAIN", None)
        if old is not None:
            os.environ["LHN_PLAIN"] = old


@pytest.mark.parametrize("setting", range(len(kc.SETTINGS)), ids=["default", "deterministic", "plain0", "plain1"])
@pytest.mark.parametrize("kind,name", CASES)
def test_route_names_every_case(kind, name, setting):
    kw = kc.SETTINGS[setting][1]
    c = kc._ALL[kind][name]
    k = kc.kernel_of(kind, name, **kw)
    assert k is not None, f"{kind}:{name}: no route"
    ch = c["cin"]
    if kind == "fwd":
        assert re.fullmatch(rf"k_w_tapmajor \+ k_kxk<{ch}, (\d), 0, 9, false>( y(\d))?", k), k
        nt, ny = int(re.search(r"<\d+, (\d)", k).group(1)), int((re.search(r" y(\d)", k) or [0, 1])[1])
        assert nt * ny == (ch + 31) // 32, k
        return
    plain = _plain_under(c, kw.get("plain"))
    assert k.startswith(DY) == plain, f"{kind}:{name} {kw}: plain_path says {plain}, the route {k}"
    assert plain or ch == 40
    p = "true" if plain else "false"
    if "nodx" in c["flags"]:
        assert "k_kxk<" not in k and "k_w_tapmajor" not in k, k
    else:
        m = re.search(rf"k_w_tapmajor \+ k_kxk<{ch}, (\d), 1, 9, {p}>( y(\d))?( par)?", k)
        assert m, k
        assert int(m.group(1)) * int(m.group(3) or 1) == (ch + 31) // 32, k
        assert bool(m.group(4)) == (c["stride"] == 2), k
    if ch == 160:
        m = re.search(rf"k_kxk_wgrad<128, (\d), 9, true> z(\d) (excl|atomic) \+ k_kxk_wgrad<32, \1, 9, true> z\2 \3$", k)
        assert m and (m.group(1), m.group(2)) in (("1", "5"), ("2", "3")), k
    else:
        assert re.search(rf"k_kxk_wgrad<40, 2, 9, {p}> (excl|atomic)$", k), k


def test_route_thresholds_at_160():
    """Five tiles in one block from 2 * cus tiles of 128 pixels on, else one tile per block; the weight gradient in five exclusive groups up
    to 16 wgrad tiles per replica, three atomic groups of two tiles past it."""
    L = kc._lib.lib()

    def q(bwd, n, h, w, nrep=4, cus=256):
        return L.lhn_conv_kxk_route(bwd, n, h, w, 160, 160, 1, nrep, kc.F_DX | kc.F_WT, cus, 0).decode()
    assert "k_kxk<160, 5, 0, 9, false>" in q(0, 1, 128, 512) and " y5" not in q(0, 1, 128, 512)          # 512 tiles
    assert "k_kxk<160, 1, 0, 9, false> y5" in q(0, 1, 128, 511)                                          # 511 tiles
    assert "k_kxk<160, 5, 1, 9, true>" in q(1, 1, 128, 512, nrep=16) and "k_kxk<160, 1, 1, 9, true> y5" in q(1, 1, 128, 511, nrep=16)
    assert "k_kxk<160, 5, 0, 9, false>" in q(0, 1, 4, 128, cus=2) and " y5" in q(0, 1, 3, 128, cus=2)    # 2 CUs: from 4 tiles
    assert kc.kernel_of("bwd", "cosplit_160_160").endswith("k_kxk_wgrad<128, 1, 9, true> z5 excl + k_kxk_wgrad<32, 1, 9, true> z5 excl")
    assert kc.kernel_of("bwd", "nocosplit_160_160").endswith("k_kxk_wgrad<128, 2, 9, true> z3 atomic + k_kxk_wgrad<32, 2, 9, true> z3 atomic")


@pytest.mark.parametrize("setting", range(len(kc.SETTINGS)), ids=["default", "deterministic", "plain0", "plain1"])
def test_route_refuses_mixed_pairs(setting):
    kw = kc.SETTINGS[setting][1]
    for kind, t in (("fwd", k6.FWD_REFUSE), ("bwd", k6.BWD_REFUSE)):
        for nm in t:
            assert kc.kernel_of(kind, nm, **kw) is None, f"{kind}:{nm}"


def test_route_keeps_the_pinned_refusals():
    L = kc._lib.lib()
    for ci, co, bwd_only in k6.OLD_REFUSALS:
        for bwd in (0, 1):
            for stride in (1, 2):
                for sw in (0, kc.SW_PLAIN0, kc.SW_PLAIN1):
                    r = L.lhn_conv_kxk_route(bwd, 2, 8, 8, ci, co, stride, 4, kc.F_DX | kc.F_WT, 256, sw)
                    if bwd or not bwd_only:
                        assert r is None, (ci, co, bwd, r)
    # 64 -> 40 and 256 -> 40 forward are older than the padded K = 40 and stay served by the 64- and 256-channel instances
    assert L.lhn_conv_kxk_route(0, 2, 9, 11, 64, 40, 1, 1, kc.F_WT, 256, 0).decode() == "k_w_tapmajor + k_kxk<64, 1, 0, 9, false> y2"
    assert L.lhn_conv_kxk_route(0, 2, 9, 11, 256, 40, 1, 1, kc.F_WT, 256, 0).decode() == "k_w_tapmajor + k_kxk<256, 1, 0, 9, false> y2"


def test_route_five_tiles_are_for_160_alone():
    """Cout (or Cin) of 129 .. 159 is five feature tiles with a partial last one: refused as before width 160 existed, whatever the
    map size (a five-tile rule that did not look at the pair would serve them on small maps only) and with or without dx."""
    L = kc._lib.lib()
    for ci, co in ((64, 144), (128, 136), (32, 159), (256, 129), (144, 64), (144, 144)):
        for nhw in ((2, 8, 8), (1, 128, 512), (64, 64, 64)):
            for cus in (256, 2):
                assert L.lhn_conv_kxk_route(0, *nhw, ci, co, 1, 4, kc.F_WT, cus, 0) is None, (ci, co, nhw, cus)
                for feat in (kc.F_DX | kc.F_WT, 0):
                    assert L.lhn_conv_kxk_route(1, *nhw, ci, co, 1, 4, feat, cus, 0) is None, (ci, co, nhw, cus, feat)
