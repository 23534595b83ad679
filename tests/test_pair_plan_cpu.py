"""CPU: which ops of a plan a whole-plan run launches in pairs (lhn_*_pair, lhn_bn_finalize_pair) -- no GPU, no kernel launch.

Like the consumer-side finalizes and LHN_PW_BWD_DZ_DEAD this is decided by the plan EXECUTOR (csrc/lhn_plan.cpp: pair_at, asked here
through lhn_plan_pair), not by a pass of the plan compiler: the op lists and tests/plan_digests.json are the same with the switch on
and off.  The rule, written out a second time in pair_kind() below, walks a list left to right; an op belongs to one pair at most:

    pool / combine: ops j and j + 1 of one kind -- MAXPOOL, plain AVGPOOL (no statistics, no copy source, bins above the small-bin
        kernel's 25 pixels), EW in sum mode, MAXPOOL_BWD, EW_BWD in its leaky single- or multi-source form -- with the same mode bits
        and source count, equal geometry of every buffer and view, writes that do not meet (as data, as gradient, or through a byte
        offset; one base and pixel stride: the channel ranges decide, anything else: the address ranges) and no write of one met by a
        read of the other;
    finalize: two consecutive convolution + BatchNorm ops of the forward list that both keep their separate finalize launch (NHWC,
        statistics, a table, no padded channel count, not evaluated twice, not handed to the next convolution:
        lhn_plan_fwd_fin_consumer, which tests/test_fwd_fin_plan_cpu.py checks), the second reading no channel of the first one's
        output view, with separate BatchNorms.

Variant B at 256 x 256 and batch 64: the 15 pool / combine pairs of the two-part RepBasicUnit outputs (PAIRS_B_*) and the 4 pairs of
depthwise branches of the MSRB rounds.  LHN_PAIR_LAUNCH=0 (read once per process: child processes here): 0 everywhere."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ENV_OFF = ("LHN_PAIR_LAUNCH", "LHN_FWD_FIN_CONSUMER", "LHN_FUSE_FINALIZE", "LHN_DW_GATHER", "LHN_PW_LDSW")
STEM, PW, DW, KXK, EW, MAXPOOL, AVGPOOL = 1, 2, 3, 4, 6, 7, 8
EW_BWD, MAXPOOL_BWD = 106, 107
TABLE_FILL, FINALIZE = 10, 5
SILU, RELU_SIGMOID = 2.0, 3.0
# variant B, batch 64.  Forward: index among the ops that are neither FINALIZE nor TABLE_FILL -> (kind, height of the source map,
# height of the destination map); backward: list position -> (kind, EW_BWD form, height of the map whose gradient is written)
PAIRS_B_FWD = {27: (MAXPOOL, 64, 32), 33: (MAXPOOL, 32, 16), 39: (MAXPOOL, 16, 8), 49: (AVGPOOL, 64, 8),
               51: (EW, 8, 8), 53: (EW, 8, 16), 59: (EW, 16, 32), 65: (EW, 32, 64)}
PAIRS_B_BWD = {34: (EW_BWD, 0, 32), 44: (EW_BWD, 0, 16), 54: (EW_BWD, 0, 8), 56: (EW_BWD, 3, 8),
               74: (MAXPOOL_BWD, 0, 16), 84: (MAXPOOL_BWD, 0, 32), 94: (MAXPOOL_BWD, 0, 64)}


def _region(base, pix, cs, coff, c):
    return (int(base), int(pix), int(cs), int(coff), int(c))


def _meet(a, b):
    if a[0] < 0 or b[0] < 0:
        return False
    if a[0] == b[0] and a[2] == b[2]:
        return a[3] < b[3] + b[4] and b[3] < a[3] + a[4]
    alo, ahi = a[0] + 4 * a[3], a[0] + 4 * ((a[1] - 1) * a[2] + a[3] + a[4])
    blo, bhi = b[0] + 4 * b[3], b[0] + 4 * ((b[1] - 1) * b[2] + b[3] + b[4])
    return alo < bhi and blo < ahi


def _access(cb, o):
    """(reads, writes) of a pool / combine op, or None when its form has no two-job kernel."""
    def data(buf, coff, c):
        b = cb[buf]
        return _region(b.data_off, b.N * b.H * b.W, b.C, coff, c)

    def grad(buf, coff, c):
        b = cb[buf]
        return _region(b.grad_off, b.N * b.H * b.W, b.C, coff, c)

    if o.out_buf < 0 and o.kind != AVGPOOL:
        return None
    if o.kind == MAXPOOL:
        return None if o.in_buf[0] < 0 else ([data(o.in_buf[0], o.in_coff[0], o.in_C[0])], [data(o.out_buf, o.out_coff, o.out_C)])
    if o.kind == EW:
        if not 1 <= o.i[0] <= 3 or o.i[2] != 0 or any(o.in_buf[k] < 0 for k in range(o.i[0])):
            return None
        return [data(o.in_buf[k], o.in_coff[k], o.in_C[k]) for k in range(o.i[0])], [data(o.out_buf, o.out_coff, o.out_C)]
    if o.kind == AVGPOOL:
        if o.in_buf[0] < 0 or o.ws[0] < 0 or o.ws[1] >= 0 or o.in_buf[1] >= 0:
            return None
        b, oh, ow = cb[o.in_buf[0]], o.i[0], o.i[1]
        if oh < 1 or ow < 1 or ((b.H + oh - 1) // oh + 1) * ((b.W + ow - 1) // ow + 1) <= 25:
            return None
        return ([data(o.in_buf[0], o.in_coff[0], o.in_C[0])],
                [_region(o.ws[0], b.N * oh * ow, o.i[3] if o.i[3] > 0 else o.in_C[0], o.i[4], o.in_C[0])])
    if o.kind == MAXPOOL_BWD:
        if o.in_buf[0] < 0:
            return None
        xb = cb[o.in_buf[0]]
        rd = [data(o.in_buf[0], o.in_coff[0], o.in_C[0]), grad(o.out_buf, o.out_coff, o.out_C)]
        if o.ws[2] >= 0:
            rd.append(_region(o.ws[2], xb.N * xb.H * xb.W, o.i[1], o.i[2], o.in_C[0]))
        if o.ws[3] >= 0:
            rd.append(_region(o.ws[3], xb.N * (o.i[7] >> 16) * (o.i[7] & 0xffff), o.i[3], o.i[6], o.in_C[0]))
        return rd, [grad(o.in_buf[0], o.in_coff[0], o.in_C[0])]
    if o.kind == EW_BWD:
        if o.i[1] not in (0, 3) or o.f[0] in (SILU, RELU_SIGMOID):
            return None
        rd, wr = [data(o.out_buf, o.out_coff, o.out_C), grad(o.out_buf, o.out_coff, o.out_C)], []
        for k in range(3 if o.i[1] == 3 else 1):
            if o.in_buf[k] < 0:
                break
            rd.append(data(o.in_buf[k], o.in_coff[k], o.in_C[k]))
            wr.append(grad(o.in_buf[k], o.in_coff[k], o.in_C[k]))
        return (rd, wr) if wr else None
    return None


def _keeps_finalize(pb, cb, ops, n, j, forward_fin):
    o = ops[j]
    has_bn = o.p[2] >= 0 or o.p[3] >= 0 or o.ws[1] >= 0
    if o.kind not in (STEM, PW, DW, KXK) or (o.kind == KXK and o.i[1] == 1) or not has_bn or o.ws[0] < 0 or o.out_buf < 0:
        return False
    if cb[o.out_buf].table_off < 0 or (o.kind == PW and (o.i[1] or o.i[2] > 0)) or (o.kind in (PW, DW) and int(o.f[3]) > 1):
        return False
    return not forward_fin(pb, ops, n, j)


def _same_shape(cb, a, b):
    if (a < 0) != (b < 0):
        return False
    return a < 0 or (cb[a].N, cb[a].H, cb[a].W) == (cb[b].N, cb[b].H, cb[b].W)


def pair_kind(pb, cb, ops, n, j, forward, forward_fin):
    """0: ops j and j + 1 launch on their own, 1: a pool / combine pair, 2: a finalize pair."""
    if j + 1 >= n:
        return 0
    a, b = ops[j], ops[j + 1]
    if forward and _keeps_finalize(pb, cb, ops, n, j, forward_fin) and _keeps_finalize(pb, cb, ops, n, j + 1, forward_fin):
        for k in range(3):
            if b.in_buf[k] == a.out_buf and b.in_coff[k] < a.out_coff + a.out_C and a.out_coff < b.in_coff[k] + b.in_C[k]:
                return 0
        if b.kind == STEM or (a.out_buf == b.out_buf and a.out_coff < b.out_coff + b.out_C and b.out_coff < a.out_coff + a.out_C):
            return 0
        if any(a.p[k] >= 0 and a.p[k] == b.p[k] for k in range(2, 7)) or a.ws[0] == b.ws[0] or (a.ws[1] >= 0 and a.ws[1] == b.ws[1]):
            return 0
        return 2
    if a.kind != b.kind:
        return 0
    if a.kind == EW and (a.i[0] != b.i[0] or a.i[2] != b.i[2]):
        return 0
    if (a.kind == EW_BWD and a.i[1] != b.i[1]) or (a.kind == AVGPOOL and (a.i[0] != b.i[0] or a.i[1] != b.i[1])):
        return 0
    if a.out_C != b.out_C or not _same_shape(cb, a.out_buf, b.out_buf):
        return 0
    for k in range(3):
        if not _same_shape(cb, a.in_buf[k], b.in_buf[k]) or (a.in_buf[k] >= 0 and a.in_C[k] != b.in_C[k]):
            return 0
    A, B = _access(cb, a), _access(cb, b)
    if A is None or B is None:
        return 0
    if any(_meet(w, q) for w in A[1] for q in B[1] + B[0]) or any(_meet(w, q) for w in B[1] for q in A[0]):
        return 0
    return 1


def rule(pb, cb, ops, n, forward, forward_fin):
    """Per op: 0, 1 (first of a pair) or 2 (second); and the kind of pair each first op starts."""
    out, kinds = [0] * n, {}
    for j in range(n - 1):
        if out[j]:
            continue
        k = pair_kind(pb, cb, ops, n, j, forward, forward_fin)
        if k:
            out[j], out[j + 1] = 1, 2
            kinds[j] = k
    return out, kinds


def _build_b64():
    from litehandnet_amd import get_model
    from litehandnet_amd.config import litehandnet_cfg
    from litehandnet_amd.plan import PlanBuilder
    cfg = litehandnet_cfg("B", image_size=256)
    cfg.MODEL["ca_dropout"] = 0.0
    m = get_model(cfg)
    tensors = list(m.state_dict(keep_vars=True).values())
    pb = PlanBuilder(64, {id(t): j for j, t in enumerate(tensors)}, image_hw=(256, 256), with_backward=True, p_drop=0.0)
    y = m.emit(pb, pb.image())
    if getattr(y, "buf", None) != -2:      # (as plan_digest.build: the NCHW head has written the output already)
        pb.set_output(y)
    return pb


def probe(name):
    import hashlib
    import plan_digest as pd
    from litehandnet_amd import _lib
    infer = name in pd.INFER_CONFIGS
    with pd.switches(name if name != "B_bs64" else "B_bwd"):
        pb = _build_b64() if name == "B_bs64" else pd.build(name)
        cb, cf, cbw, nf, nb = pb.finalize()
    h = hashlib.sha256()
    for a in (cb, cf) + ((cbw,) if nb else ()):
        h.update(pd._raw(a))
    h.update(pd._tail(pb).encode())
    L = _lib.lib()
    L.lhn_plan_pair.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.lhn_plan_pair.restype = C.c_int
    L.lhn_plan_fwd_fin_consumer.argtypes = [C.c_void_p, C.c_int]
    L.lhn_plan_fwd_fin_consumer.restype = C.c_int
    p = L.lhn_plan_create(cb, len(pb.bufs), cf, nf, cbw, nb)
    assert p, L.lhn_last_error().decode()
    try:
        got = [[L.lhn_plan_pair(C.c_void_p(p), ph, j) for j in range(n)] for ph, n in ((0, nf), (1, nb))]
        edge = [L.lhn_plan_pair(C.c_void_p(p), 0, -1), L.lhn_plan_pair(C.c_void_p(p), 0, nf), L.lhn_plan_pair(C.c_void_p(p), 1, nb),
                L.lhn_plan_pair(C.c_void_p(p), 2, 0), L.lhn_plan_pair(C.c_void_p(p), -1, 0)]
        handed = [L.lhn_plan_fwd_fin_consumer(C.c_void_p(p), j) == 1 for j in range(nf)]
    finally:
        L.lhn_plan_destroy(C.c_void_p(p))
    # which finalizes are handed to the next convolution is the executor's own answer: tests/test_fwd_fin_plan_cpu.py checks it
    fin = lambda pb_, ops, n, j: handed[j]      # noqa: E731
    wf, kf = rule(pb, cb, cf, nf, True, fin)
    wb, kb = rule(pb, cb, cbw, nb, False, fin) if nb else ([], {})
    # forward positions among the ops that are neither FINALIZE nor TABLE_FILL
    pos, k = {}, 0
    for j in range(nf):
        pos[j] = k
        k += cf[j].kind not in (FINALIZE, TABLE_FILL)
    H = lambda buf: int(cb[buf].H)      # noqa: E731
    fwd_pool = {pos[j]: [cf[j].kind, H(cf[j].in_buf[0]), H(cf[j].out_buf) if cf[j].kind != AVGPOOL else int(cf[j].i[0])]
                for j in range(nf) if got[0][j] == 1 and cf[j].kind in (EW, MAXPOOL, AVGPOOL)}
    fwd_fin = [[cf[j].kind, cf[j + 1].kind, H(cf[j].out_buf)] for j in range(nf) if got[0][j] == 1 and cf[j].kind in (STEM, PW, DW, KXK)]
    bwd_pool = {j: [cbw[j].kind, int(cbw[j].i[1]) if cbw[j].kind == EW_BWD else 0, H(cbw[j].in_buf[0])] for j in range(nb) if got[1][j] == 1}
    other = [j for j in range(nf) if got[0][j] == 1 and cf[j].kind not in (EW, MAXPOOL, AVGPOOL, STEM, PW, DW, KXK)]
    return dict(got=got, want=[wf, wb], edge=edge, fwd_pool={str(k): v for k, v in fwd_pool.items()}, fwd_fin=fwd_fin,
                bwd_pool={str(k): v for k, v in bwd_pool.items()}, other=other, infer=infer, sha256=h.hexdigest())


def _names():
    with open(os.path.join(HERE, "plan_digests.json")) as f:
        return sorted(json.load(f)["configs"])


CONFIGS = _names()


def _child(names, **env_extra):
    env = {k: v for k, v in os.environ.items() if k not in ENV_OFF}
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + list(names), env=dict(env, **env_extra), capture_output=True, text=True,
                       timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def probed():
    return _child(CONFIGS + ["B_bs64"])


@pytest.fixture(scope="module")
def probed_off():
    return _child(["B_bwd", "B_bs64"], LHN_PAIR_LAUNCH="0")


@pytest.mark.parametrize("name", CONFIGS)
def test_executor_names_the_pairs_of_the_rule(probed, name):
    r = probed[name]
    assert r["got"] == r["want"] and r["edge"] == [-1, -1, -1, -1, -1] and r["other"] == []
    for lst in r["got"]:      # every first op is followed by its second, and nothing else is marked
        assert all((v == 1) == (j + 1 < len(lst) and lst[j + 1] == 2) for j, v in enumerate(lst)) and set(lst) <= {0, 1, 2}
    with open(os.path.join(HERE, "plan_digests.json")) as f:
        assert r["sha256"] == json.load(f)["configs"][name]["sha256"]          # the op lists are what they were


def test_variant_b_at_batch_64_pairs_15_pool_and_combine_launches_and_4_finalizes(probed):
    r = probed["B_bs64"]
    assert r["got"] == r["want"]
    assert {int(k): tuple(v) for k, v in r["fwd_pool"].items()} == PAIRS_B_FWD
    assert {int(k): tuple(v) for k, v in r["bwd_pool"].items()} == PAIRS_B_BWD
    assert len(PAIRS_B_FWD) + len(PAIRS_B_BWD) == 15
    assert r["fwd_fin"] == [[DW, DW, 64]] * 4                 # the two depthwise branches of each MSRB round
    assert sum(v == 1 for lst in r["got"] for v in lst) == 19
    # the batch size moves offsets, not pairs
    assert (probed["B_bwd"]["fwd_pool"], probed["B_bwd"]["bwd_pool"], probed["B_bwd"]["fwd_fin"]) == (r["fwd_pool"], r["bwd_pool"], r["fwd_fin"])


@pytest.mark.parametrize("name", ["B_bwd", "B_bs64"])
def test_switch_off_pairs_nothing_and_leaves_the_op_lists(probed, probed_off, name):
    r = probed_off[name]
    assert all(v == 0 for lst in r["got"] for v in lst) and r["edge"] == [-1, -1, -1, -1, -1]
    assert sum(v == 1 for lst in r["want"] for v in lst) == 19
    assert r["sha256"] == probed[name]["sha256"]
    if name == "B_bwd":
        with open(os.path.join(HERE, "plan_digests.json")) as f:
            assert r["sha256"] == json.load(f)["configs"][name]["sha256"]


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    print(json.dumps({n: probe(n) for n in sys.argv[1:]}))
