"""Digests of the op lists PlanBuilder.finalize() hands to lhn_plan_create, for a fixed set of plans -- no GPU, no kernel launch.

tests/plan_digests.json pins them as the plan compiler produced them at the commit named in its "generated_at" field;
tests/test_plan_digest_cpu.py compares every configuration against that file.  The file is never regenerated to make a
change of plan.py pass: a changed hash means changed launches.

tests/plan_digests_infer.json does the same for plans without a backward under the six inference switches (INFER_CONFIGS), in eval
form and in deployed form, with the pass counters next to each hash.  The same rule holds for it.

    python tests/plan_digest.py --write FILE          all records of CONFIGS as JSON
    python tests/plan_digest.py --write-infer FILE    all records of INFER_CONFIGS as JSON
    python tests/plan_digest.py --dump CONFIG         one line per buffer / op with every slot (diff two trees as text)
"""
import argparse
import contextlib
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SWITCHES = ("LHN_COPY_POOL", "LHN_GATE_BN_SUMS", "LHN_SUM_OUT", "LHN_GRAD_ADDENDS", "LHN_FUSE_BN_SUMS", "LHN_READER_BN_SUMS",
            "LHN_POOL_GRAD_ADDS", "LHN_EW_BWD_MULTI")
# The PlanBuilder keyword of each inference switch, in the order finalize() runs the passes, and the counter its pass bumps.
INFER_KW = ("infer_fuse_stem", "infer_fuse_msrb", "infer_fuse_dwpw", "infer_fuse", "infer_fuse_bneck", "infer_bf16x3")
INFER_COUNTERS = ("n_fused", "n_fused_dwpw", "n_fused_msrb", "n_fused_bneck", "n_fused_stem", "n_bf16x3")
INFER_COUNTER_OF = dict(zip(INFER_KW, ("n_fused_stem", "n_fused_msrb", "n_fused_dwpw", "n_fused", "n_fused_bneck", "n_bf16x3")))
INFER_ENV = ("LHN_INFER_FUSE", "LHN_INFER_FUSE_DWPW", "LHN_INFER_FUSE_MSRB", "LHN_INFER_FUSE_BNECK", "LHN_INFER_BF16X3", "LHN_INFER_FUSE_STEM")
COUNTERS = ("grad_aliases", "grad_addends", "fused_bn_sums", "reader_bn_sums", "pool_grad_adds", "ew_bwd_multi")


def _configs():
    """name -> dict(variant | block, size, backward, model_kw, off (switches set to "0"), infer_fuse); all at N = 2."""
    out = {}

    def add(name, **kw):
        out[name] = dict(dict(variant=None, block=None, size=256, backward=True, model_kw={}, off=(), infer_fuse=False), **kw)

    for v in "ABMHL":
        add(f"{v}_bwd", variant=v)
        add(f"{v}_fwd", variant=v, backward=False)
    add("B_224_bwd", variant="B", size=224)
    add("B_se_bwd", variant="B", model_kw=dict(msrb_ca="se", rbu_ca="se"))
    add("A_silu_bwd", variant="A", model_kw=dict(activation="silu"))
    for s in SWITCHES:
        add(f"B_bwd_{s}=0", variant="B", off=(s,))
    add("B_bwd_all_off", variant="B", off=SWITCHES)
    add("A_bwd_LHN_EW_BWD_MULTI=0", variant="A", off=("LHN_EW_BWD_MULTI",))
    add("M_bwd_LHN_EW_BWD_MULTI=0", variant="M", off=("LHN_EW_BWD_MULTI",))
    for v in "ABM":
        add(f"{v}_fwd_eval_fused", variant=v, backward=False, infer_fuse=True)
    add("block_RepBasicUnit_bwd", block="RepBasicUnit", size=16)
    add("block_MSRB_bwd", block="MSRB", size=16)
    return out


CONFIGS = _configs()


def _infer_configs():
    """name -> dict(variant, size, deployed, model_kw, on (the INFER_KW passed as True; the rest are passed as False)); all at N = 2,
    no backward.  A, B and M in both forms with each switch alone and with all six, A and B at 224 (ragged tiles: the same ops over
    another shape), and the other model families in eval form with all six."""
    out = {}

    def add(name, **kw):
        out[name] = dict(dict(size=256, deployed=False, model_kw={}, on=INFER_KW), **kw)

    for v in "ABM":
        for deployed in (False, True):
            form = "deployed" if deployed else "eval"
            for kw in INFER_KW:
                add(f"{v}_{form}_{kw}", variant=v, deployed=deployed, on=(kw,))
            add(f"{v}_{form}_all", variant=v, deployed=deployed)
            if v in "AB":
                add(f"{v}_224_{form}_all", variant=v, deployed=deployed, size=224)
    add("H_eval_all", variant="H")
    add("L_eval_all", variant="L")
    add("X_cbam_msrb_eval_all", variant="X", model_kw=dict(ca_type="cbam", msrb=True))
    return out


INFER_CONFIGS = _infer_configs()


def _deploy_without_gpu(m):
    """The deployed module tree of m, built in place without the GPU fold: every RepConv, RepBlock and ChannelAttension gets the single
    biased convolution deploy() would leave (weights are whatever nn.Conv2d draws: the plan compiler looks at shapes)."""
    from torch import nn
    for u in m.modules():
        if hasattr(u, "conv") and hasattr(u, "slope") and not hasattr(u, "rep_conv"):
            c = u.conv.conv
            u.rep_conv = nn.Conv2d(c.in_channels, c.out_channels, c.kernel_size, c.stride, c.padding, c.dilation, c.groups, bias=True)
            del u.conv
        if hasattr(u, "rbr_dense"):
            c = u.rbr_dense.conv
            u.rbr_reparam = nn.Conv2d(c.in_channels, c.out_channels, c.kernel_size, c.stride, c.padding, c.dilation, c.groups, bias=True)
            del u.rbr_dense, u.rbr_1x1
            if hasattr(u, "rbr_identity"):
                del u.rbr_identity
        if hasattr(u, "conv3x3") and not hasattr(u, "rbr_reparam"):
            c = u.conv3x3.conv
            u.rbr_reparam = nn.Conv2d(c.in_channels, c.out_channels, 3, 1, 0, groups=c.groups)
            del u.conv3x3
    return m


def build(name):
    """The PlanBuilder of configuration `name`, emitted and not yet finalized.  The plan switches are read from the
    environment while this runs and while finalize() runs: the caller sets them (see switches())."""
    from litehandnet_amd import get_model, litehourglass
    from litehandnet_amd.config import litehandnet_cfg
    from litehandnet_amd.plan import PlanBuilder
    if name in INFER_CONFIGS:
        c = INFER_CONFIGS[name]
        size = c["size"]
        cfg = litehandnet_cfg(c["variant"], image_size=size, **c["model_kw"])
        cfg.MODEL["ca_dropout"] = 0.0
        m = get_model(cfg).eval()
        if c["deployed"]:
            _deploy_without_gpu(m)
        tensors = list(m.state_dict(keep_vars=True).values())
        pb = PlanBuilder(2, {id(t): j for j, t in enumerate(tensors)}, image_hw=(size, size), with_backward=False, p_drop=0.0,
                         **{kw: kw in c["on"] for kw in INFER_KW})
        pb.set_output(m.emit(pb, pb.image()))
        return pb
    c = CONFIGS[name]
    size = c["size"]
    if c["block"]:
        m = getattr(litehourglass, c["block"])(128, 128, "ca", p_drop=0.0)
    else:
        cfg = litehandnet_cfg(c["variant"], image_size=size, **c["model_kw"])
        cfg.MODEL["ca_dropout"] = 0.0
        m = get_model(cfg)
    if c["infer_fuse"]:
        m.eval()
    tensors = list(m.state_dict(keep_vars=True).values())
    pb = PlanBuilder(2, {id(t): j for j, t in enumerate(tensors)}, image_hw=(size, size), with_backward=c["backward"], p_drop=0.0,
                     infer_fuse=c["infer_fuse"])
    y = m.emit(pb, pb.input_tensor(128, size, size) if c["block"] else pb.image())
    if getattr(y, "buf", None) != -2:
        pb.set_output(y)
    return pb


@contextlib.contextmanager
def switches(name):
    """The environment of configuration `name` for a script run (the tests use monkeypatch instead)."""
    saved = {s: os.environ.get(s) for s in SWITCHES + INFER_ENV}
    try:
        for s in saved:
            os.environ.pop(s, None)
        for s in CONFIGS[name]["off"] if name in CONFIGS else ():
            os.environ[s] = "0"
        yield
    finally:
        for s, v in saved.items():
            os.environ.pop(s, None)
            if v is not None:
                os.environ[s] = v


def _raw(arr):
    return b"" if arr is None else C.string_at(C.addressof(arr), C.sizeof(arr))


def _tail(pb):
    counters = tuple(getattr(pb, k, 0) for k in COUNTERS) if pb.with_backward else ()
    return repr((pb.sync_points, pb.n_fused, counters))


def digest(pb):
    """finalize() the built PlanBuilder and return {n_fwd, n_bwd, total_bytes, act_bytes, sha256}.  The hash covers the Buf
    array, the forward Op array, the backward Op array (if any) and repr((sync_points, n_fused, counters))."""
    cb, cf, cbw, nf, nb = pb.finalize()
    h = hashlib.sha256()
    h.update(_raw(cb))
    h.update(_raw(cf))
    if nb:
        h.update(_raw(cbw))
    h.update(_tail(pb).encode())
    return dict(n_fwd=nf, n_bwd=nb, total_bytes=pb.total_bytes, act_bytes=pb.act_bytes, sha256=h.hexdigest())


def infer_digest(pb):
    """finalize() the built inference PlanBuilder and return {n_fwd, total_bytes, act_bytes, counters, sha256}.  The hash covers the
    Buf array, the forward Op array, repr of the six counters (in the order of INFER_COUNTERS), total_bytes and act_bytes."""
    cb, cf, cbw, nf, nb = pb.finalize()
    assert nb == 0
    counters = {k: getattr(pb, k) for k in INFER_COUNTERS}
    h = hashlib.sha256()
    h.update(_raw(cb))
    h.update(_raw(cf))
    h.update(repr((tuple(counters.values()), pb.total_bytes, pb.act_bytes)).encode())
    return dict(n_fwd=nf, total_bytes=pb.total_bytes, act_bytes=pb.act_bytes, counters=counters, sha256=h.hexdigest())


def dump(pb, out=sys.stdout):
    cb, cf, cbw, nf, nb = pb.finalize()
    for j in range(len(pb.bufs)):
        b = cb[j]
        out.write(f"buf {j}: data={b.data_off} table={b.table_off} gate={b.gate_off} grad={b.grad_off} dpool={b.dpool_off} "
                  f"coef={b.coef_off} NHWC={b.N},{b.H},{b.W},{b.C}\n")
    for tag, arr, n in (("fwd", cf, nf), ("bwd", cbw, nb)):
        for j in range(n):
            o = arr[j]
            out.write(f"{tag} {j}: kind={o.kind} in_buf={list(o.in_buf)} in_coff={list(o.in_coff)} in_C={list(o.in_C)} "
                      f"out={o.out_buf},{o.out_coff},{o.out_C} p={list(o.p)} ws={list(o.ws)} i={list(o.i)} "
                      f"f={[float(v).hex() for v in o.f]}\n")
    out.write(f"total_bytes={pb.total_bytes} act_bytes={pb.act_bytes}\n{_tail(pb)}\n")
    out.write(" ".join(f"{k}={getattr(pb, k)}" for k in INFER_COUNTERS) + "\n")


def record(name):
    with switches(name):
        return (infer_digest if name in INFER_CONFIGS else digest)(build(name))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--write", metavar="FILE")
    ap.add_argument("--write-infer", metavar="FILE")
    ap.add_argument("--dump", metavar="CONFIG", choices=sorted(CONFIGS) + sorted(INFER_CONFIGS))
    ap.add_argument("--generated-at", default="", help="commit whose plan.py produced the records (stored in the file)")
    a = ap.parse_args()
    if a.dump:
        with switches(a.dump):
            dump(build(a.dump))
    for path, table in ((a.write, CONFIGS), (a.write_infer, INFER_CONFIGS)):
        if path:
            doc = {"generated_at": a.generated_at, "configs": {name: record(name) for name in table}}
            with open(path, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
