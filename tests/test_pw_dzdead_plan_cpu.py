"""CPU: which 1x1 backward ops of a training plan run without their dy store (LHN_PW_BWD_DZ_DEAD of lhn_conv_pw_bwd6) -- no GPU, no
kernel launch.

The decision is taken by the plan EXECUTOR (csrc/lhn_plan.cpp: pw_dz_dead_at, asked here through lhn_plan_pw_dz_dead), not by the plan
compiler: the op lists of tests/plan_digests.json do not change.  An op takes the flag when nothing behind it in the backward list
touches the gradient of its output view.  This test scans the same lists on its own and names what it finds:

  * A, B, M, L, the B switch configurations and the two blocks: no op behind any NHWC PW_BWD touches its output's gradient, so every
    one of them takes the flag.  B has three wide ones (k_pw_bwd_wr: the two MSRB closing 128 -> 128 and the stem's 64 -> 128), the
    MSRB block one.
  * H (the stacked hourglass): conv3 and the skip 1x1 of a Residual both read d(sum) from ONE aliased gradient buffer, so the first
    of each pair has a later reader and keeps today's behaviour -- there, and in A with SiLU, the later op wants dz (which an
    in-place dy only equals because these convolutions have no BatchNorm)."""
import ctypes as C

import pytest

import plan_digest as pd

BWD_CONFIGS = [n for n, c in pd.CONFIGS.items() if c["backward"]]
WIDE = ((128, 128), (64, 128), (128, 64))
# configuration -> NHWC PW_BWD ops that keep the store because a later op touches their dz, as the lists stand
KEPT = {"H_bwd": 4, "A_silu_bwd": 3}
WIDE_FLAGGED = {"A_bwd": 8, "B_bwd": 3, "M_bwd": 6, "H_bwd": 4, "L_bwd": 0, "block_MSRB_bwd": 1, "block_RepBasicUnit_bwd": 0}


def _scan(cb, cbw, nb, j):
    """Does any op behind backward op j touch the gradient of j's output view?  (Written from the layout of the op arrays, not from
    the executor's code: gradient byte ranges of out_buf / in_buf with overlapping channels, and byte offsets in ws[].)"""
    from litehandnet_amd.plan import MEMSET

    def grad(b):
        r = cb[b]
        return (r.grad_off, r.grad_off + 4 * r.N * r.H * r.W * r.C) if b >= 0 and r.grad_off >= 0 else None

    o = cbw[j]
    lo, hi = grad(o.out_buf)
    for k in range(j + 1, nb):
        q = cbw[k]
        if q.kind == MEMSET:
            if q.ws[0] < hi and lo < q.ws[0] + q.ws[1]:
                return True
            continue
        for buf, coff, c in [(q.out_buf, q.out_coff, q.out_C)] + [(q.in_buf[s], q.in_coff[s], q.in_C[s]) for s in range(3)]:
            g = grad(buf)
            if g and g[0] < hi and lo < g[1]:
                same_layout = g[0] == lo and cb[buf].C == cb[o.out_buf].C
                if not same_layout or (coff < o.out_coff + o.out_C and o.out_coff < coff + c):
                    return True
        if any(lo <= q.ws[s] < hi for s in range(12)):
            return True
    return False


@pytest.mark.parametrize("name", BWD_CONFIGS)
def test_executor_flags_exactly_the_ops_without_a_later_reader(name, monkeypatch):
    from litehandnet_amd import _lib
    from litehandnet_amd.plan import PW_BWD
    for s in pd.SWITCHES + pd.INFER_ENV:
        monkeypatch.delenv(s, raising=False)
    for s in pd.CONFIGS[name]["off"]:
        monkeypatch.setenv(s, "0")
    pb = pd.build(name)
    cb, cf, cbw, nf, nb = pb.finalize()
    L = _lib.lib()
    L.lhn_plan_pw_dz_dead.argtypes = [C.c_void_p, C.c_int]
    L.lhn_plan_pw_dz_dead.restype = C.c_int
    h = L.lhn_plan_create(cb, len(pb.bufs), cf, nf, cbw, nb)
    assert h, L.lhn_last_error().decode()
    try:
        got = [L.lhn_plan_pw_dz_dead(C.c_void_p(h), j) for j in range(nb)]
        assert L.lhn_plan_pw_dz_dead(C.c_void_p(h), nb) == -1 and L.lhn_plan_pw_dz_dead(C.c_void_p(h), -1) == -1
    finally:
        L.lhn_plan_destroy(C.c_void_p(h))
    kept = wide = 0
    for j in range(nb):
        o = cbw[j]
        nhwc_pw = o.kind == PW_BWD and not o.i[1] and cb[o.out_buf].grad_off >= 0
        want = int(nhwc_pw and not _scan(cb, cbw, nb, j))
        assert got[j] == want, f"{name}: backward op {j} (kind {o.kind}, out {o.out_buf},{o.out_coff},{o.out_C}): executor {got[j]}, scan {want}"
        kept += int(nhwc_pw and not want)
        wide += int(want and o.i[0] == 1 and (o.in_C[0], o.out_C) in WIDE)
    assert kept == KEPT.get(name, 0), f"{name}: {kept} NHWC PW_BWD ops have a later reader of their dz"
    if name in WIDE_FLAGGED:
        assert wide == WIDE_FLAGGED[name], f"{name}: {wide} wide PW_BWD ops take the flag"
    if name.startswith("B_"):
        assert wide == 3, f"{name}: {wide} wide PW_BWD ops take the flag"
