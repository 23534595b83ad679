"""CPU: the 1x1 backward route does not know the accumulate.  An accumulating 32 -> 32 call runs the PF = 3 instances of k_pw_bwd_wr
(the prior dx in the prefetch, csrc/k_conv_pw.hip) behind the launcher of the PF = 2 instance the route names, so lhn_conv_pw_route
answers Cin = Cout in {32, 64}, with and without reader-side sums, exactly as without LHN_PW_F_DX_ACC: the strings below, which are
the ones tests/test_pw_route_cpu.py holds for the narrow instances."""
import pytest

import pw_cases as pc
from litehandnet_amd import _lib

TODAY = {(64, False): "k_pw_bwd_wr<64, 64, 64, 2, false, false, 2>", (64, True): "k_pw_bwd_wr<64, 64, 64, 2, false, true, 2>",
         (32, False): "k_pw_bwd_wr<32, 32, 128, 2, false, false, 3>", (32, True): "k_pw_bwd_wr<32, 32, 128, 2, false, true, 2>"}
SW = pc.SW_K256 | pc.SW_BWD_NARROW | pc.SW_HEAD_STREAM


def _ask(c, feat, nhw=(2, 10, 10), sw=SW):
    r = _lib.lib().lhn_conv_pw_route(1, nhw[0], nhw[1], nhw[2], c, c, 1, 0, 0, feat, sw)
    return r.decode() if r is not None else None


@pytest.mark.parametrize("bns", [False, True])
@pytest.mark.parametrize("c", [32, 64])
def test_route_ignores_dx_acc(c, bns):
    for extra in (0, pc.F_DBIAS, pc.F_FIN, pc.F_DZ_DEAD):
        for nhw in ((1, 3, 3), (2, 10, 10), (64, 128, 128)):
            feat = extra | pc.F_BNSUM * bns
            plain, acc = _ask(c, feat, nhw), _ask(c, feat | pc.F_DX_ACC, nhw)
            assert plain == acc == TODAY[(c, bns)], (c, bns, extra, nhw, plain, acc)


@pytest.mark.parametrize("c", [32, 64])
def test_route_ignores_dx_acc_under_the_switches(c):
    """Deterministic mode and LHN_PW_BWD_NARROW=0 change the answer; the accumulate flag still does not."""
    for sw in (SW | pc.SW_DETERMINISTIC, SW & ~pc.SW_BWD_NARROW, SW | pc.SW_LDSW):
        for bns in (False, True):
            feat = pc.F_BNSUM * bns
            assert _ask(c, feat, sw=sw) == _ask(c, feat | pc.F_DX_ACC, sw=sw) is not None
    assert _ask(c, 0, sw=SW & ~pc.SW_BWD_NARROW).startswith("k_pw_bwd<")
