"""CPU: which forward BatchNorm finalizes a training plan hands to the next convolution (lhn_bnfinsrc) -- no GPU, no kernel launch.

Like LHN_BWD_FIN_CONSUMER and the head's gate fold this is decided by the plan EXECUTOR (csrc/lhn_plan.cpp: fwd_fin_consumer_at, asked
here through lhn_plan_fwd_fin_consumer), not by a pass of the plan compiler: the op lists and tests/plan_digests.json are the same
with the switch on and off.  The rule, written out a second time in rule() below:

    producer: STEM / PW / DW / KXK with a BatchNorm and statistics, NHWC, no padded channel count, not evaluated twice;
    consumer: the NEXT op of the list, a single-source NHWC DW or PW whose input view is the producer's output view (buffer, first
              channel, channels), on a kernel with the prologue fold: 3x3 depthwise at stride 1 / dilation 1 / pad 1 on a map at
              least 8 wide or at stride 2 / pad 1, 1x1 at stride 1 with the whole weight, 64 -> 33..64 or 32 -> <= 32 features.

Variant B at 256 x 256: 30 of its 52 BatchNorms, by op index in PAIRS_B.  (The forward RECORDS of dump_plan.py show 29: the copy
b54[0:64] -> b57[0:64] is recorded between the depthwise b55 -> b56 and the 1x1 b56 -> b58, but stands in front of the 1x1
b54 -> b55 in the op list, so op 77 is followed by its reader directly.)  LHN_FWD_FIN_CONSUMER=0 or LHN_FUSE_FINALIZE=1 (both read
once per process: child processes here): nothing is handed over."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CONFIGS = ("A_bwd", "B_bwd", "M_bwd", "H_bwd", "L_bwd", "B_224_bwd", "block_RepBasicUnit_bwd", "block_MSRB_bwd")
ENV_OFF = ("LHN_FWD_FIN_CONSUMER", "LHN_FUSE_FINALIZE", "LHN_DW_GATHER", "LHN_PW_LDSW")
STEM, PW, DW, KXK = 1, 2, 3, 4
# variant B, 256 x 256: producer op index -> (producer kind, consumer kind, height of the map the consumer reads)
PAIRS_B = {1: (STEM, DW, 128), 2: (DW, PW, 128), 3: (PW, DW, 128), 4: (DW, PW, 64),
           8: (PW, DW, 64), 12: (PW, DW, 64), 25: (PW, DW, 64), 76: (PW, DW, 64), 77: (DW, PW, 64), 78: (PW, DW, 64), 82: (PW, DW, 64),
           29: (PW, DW, 32), 30: (DW, PW, 32), 31: (PW, DW, 32), 61: (PW, DW, 32), 62: (DW, PW, 32), 63: (PW, DW, 32),
           35: (PW, DW, 16), 36: (DW, PW, 16), 37: (PW, DW, 16), 55: (PW, DW, 16), 56: (DW, PW, 16), 57: (PW, DW, 16),
           41: (PW, DW, 8), 42: (DW, PW, 8), 43: (PW, DW, 8), 44: (DW, PW, 8), 45: (PW, DW, 8), 46: (DW, PW, 8), 47: (PW, DW, 8)}


def rule(pb, cf, nf, j):
    if j + 1 >= nf:
        return False
    o, q = cf[j], cf[j + 1]
    has_bn = o.p[2] >= 0 or o.p[3] >= 0 or o.ws[1] >= 0
    if o.kind not in (STEM, PW, DW, KXK) or not has_bn or o.ws[0] < 0 or (o.kind == KXK and o.i[1] == 1):
        return False
    if (o.kind == PW and (o.i[1] or o.i[2] > 0)) or (o.kind in (PW, DW) and int(o.f[3]) > 1):
        return False
    if q.kind not in (DW, PW) or q.i[6] > 1 or (q.in_buf[0], q.in_coff[0], q.in_C[0]) != (o.out_buf, o.out_coff, o.out_C):
        return False
    b = pb.bufs[o.out_buf]
    if q.kind == DW:
        k, s, p, d = q.i[0], q.i[1], q.i[2], q.i[3]
        return q.p[0] >= 0 and k == 3 and p == 1 and d == 1 and ((s == 1 and b.W >= 8) or s == 2)
    cin, cout = q.in_C[0], q.out_C
    whole = q.i[2] in (0, cout) and q.i[3] in (0, cin)
    return not q.i[1] and q.i[0] == 1 and whole and ((cin == 64 and 32 < cout <= 64) or (cin == 32 and cout <= 32))


def probe(name):
    import plan_digest as pd
    from litehandnet_amd import _lib
    with pd.switches(name):
        pb = pd.build(name)
        cb, cf, cbw, nf, nb = pb.finalize()
    import hashlib
    h = hashlib.sha256()
    for a in (cb, cf) + ((cbw,) if nb else ()):
        h.update(pd._raw(a))
    h.update(pd._tail(pb).encode())
    L = _lib.lib()
    L.lhn_plan_fwd_fin_consumer.argtypes = [C.c_void_p, C.c_int]
    L.lhn_plan_fwd_fin_consumer.restype = C.c_int
    p = L.lhn_plan_create(cb, len(pb.bufs), cf, nf, cbw, nb)
    assert p, L.lhn_last_error().decode()
    try:
        got = [j for j in range(nf) if L.lhn_plan_fwd_fin_consumer(C.c_void_p(p), j) == 1]
        edge = [L.lhn_plan_fwd_fin_consumer(C.c_void_p(p), -1), L.lhn_plan_fwd_fin_consumer(C.c_void_p(p), nf)]
    finally:
        L.lhn_plan_destroy(C.c_void_p(p))
    want = [j for j in range(nf) if rule(pb, cf, nf, j)]
    kinds = {j: (cf[j].kind, cf[j + 1].kind, pb.bufs[cf[j].out_buf].H) for j in got}
    nbn = sum(1 for j in range(nf) if cf[j].kind in (STEM, PW, DW, KXK) and (cf[j].p[2] >= 0 or cf[j].p[3] >= 0 or cf[j].ws[1] >= 0))
    return dict(got=got, want=want, edge=edge, kinds={str(j): list(v) for j, v in kinds.items()}, nbn=nbn, sha256=h.hexdigest())


def _child(names, **env_extra):
    env = {k: v for k, v in os.environ.items() if k not in ENV_OFF}
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + list(names), env=dict(env, **env_extra), capture_output=True, text=True,
                       timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def probed():
    return _child(CONFIGS)


@pytest.mark.parametrize("name", CONFIGS)
def test_executor_names_the_pairs_of_the_rule(probed, name):
    r = probed[name]
    assert r["got"] == r["want"] and r["edge"] == [-1, -1]
    with open(os.path.join(HERE, "plan_digests.json")) as f:
        assert r["sha256"] == json.load(f)["configs"][name]["sha256"]          # the op lists are what they were


def test_variant_b_hands_over_30_of_52(probed):
    r = probed["B_bwd"]
    assert r["nbn"] == 52 and r["got"] == sorted(PAIRS_B)
    assert {int(j): tuple(v) for j, v in r["kinds"].items()} == PAIRS_B


@pytest.mark.parametrize("env", [{"LHN_FWD_FIN_CONSUMER": "0"}, {"LHN_FUSE_FINALIZE": "1"}])
def test_switch_off_or_producer_side_fusion_hands_nothing_over(env):
    r = _child(["B_bwd"], **env)["B_bwd"]
    assert r["got"] == [] and len(r["want"]) == 30


def test_routes_name_the_folding_instance_or_the_launch_in_front():
    from litehandnet_amd import _lib
    L = _lib.lib()
    FS_DW, FS_PW, STATS = 128, 16384, 2
    dw = lambda h, w, c, k, s, p, d, f=FS_DW, sw=4: (lambda r: r.decode() if r is not None else None)(      # noqa: E731
        L.lhn_conv_dw_route(0, h, w, c, k, s, p, d, f, sw))
    pw = lambda cin, cout, f=FS_PW | STATS, sw=2 | 4 | 16, stride=1: (lambda r: r.decode() if r is not None else None)(      # noqa: E731
        L.lhn_conv_pw_route(0, 2, 16, 16, cin, cout, stride, 0, 0, f, sw))
    assert dw(64, 64, 64, 3, 1, 1, 1) == "k_dwk_fwd_lds<3,1,1,true>"
    assert dw(8, 8, 32, 3, 1, 1, 1) == "k_dwk_fwd_lds<3,1,1,true>"
    assert dw(16, 16, 80, 3, 2, 1, 1) == "k_dws2_fwd_lds<true>"
    assert dw(4, 4, 64, 3, 1, 1, 1) == "lhn_bn_finalize + k_dw_fwd<3>"                      # W < 8
    assert dw(32, 32, 64, 3, 1, 2, 2) == "lhn_bn_finalize + k_dwk_fwd_lds<3,1> ps=2"
    assert dw(12, 12, 64, 3, 1, 2, 2) == "lhn_bn_finalize + k_dwk_fwd_lds<3,2>"
    assert dw(16, 16, 32, 7, 1, 3, 1) == "lhn_bn_finalize + k_dwk_fwd_lds<7,1>"
    assert dw(16, 16, 32, 3, 1, 1, 1, FS_DW | 2) == "lhn_bn_finalize + k_dwk_fwd_lds<3,1,2>"   # a second source never folds
    assert dw(16, 16, 32, 3, 1, 1, 1, FS_DW, 4 | 1) == "lhn_bn_finalize + k_dw_fwd<3>"         # LHN_DW_GATHER=1
    assert dw(64, 64, 64, 3, 1, 1, 1, 0) == "k_dwk_fwd_lds<3,1>" and dw(16, 16, 32, 3, 2, 1, 1, 0) == "k_dws2_fwd_lds"
    assert pw(64, 64) == "k_pw_fwd_wr<64, 2, 1, true>" and pw(64, 48) == "k_pw_fwd_wr<64, 2, 1, true>"
    assert pw(32, 32) == "k_pw_fwd_wr<32, 1, 1, true>"
    assert pw(64, 32) == "lhn_bn_finalize + k_pw_fwd_wr<64, 1, 1>"
    assert pw(64, 128) == "lhn_bn_finalize + k_pw_fwd_wr<64, 4, 1>"
    assert pw(128, 128) == "lhn_bn_finalize + k_pw_fwd_wr<128, 4, 1>"
    assert pw(32, 64) == "lhn_bn_finalize + k_pw_fwd_wr<32, 2, 1>"
    assert pw(64, 64, sw=1 | 2 | 4 | 16) == "lhn_bn_finalize + k_pw_fwd<64, 2, 1>"             # LHN_PW_LDSW=1
    assert pw(64, 64, stride=2) == "lhn_bn_finalize + k_pw_fwd<64, 2, 1>"
    assert pw(64, 64, STATS) == "k_pw_fwd_wr<64, 2, 1>" and pw(32, 32, STATS) == "k_pw_fwd_wr<32, 1, 1>"


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    print(json.dumps({n: probe(n) for n in sys.argv[1:]}))
