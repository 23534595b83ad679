"""Digests of the op lists PlanBuilder.finalize() hands to lhn_plan_create, for a fixed set of plans -- no GPU, no kernel launch.

tests/plan_digests.json pins them as the plan compiler produced them at the commit named in its "generated_at" field;
tests/test_plan_digest_cpu.py compares every configuration against that file.  The file is never regenerated to make a
change of plan.py pass: a changed hash means changed launches.

    python tests/plan_digest.py --write FILE       all records as JSON
    python tests/plan_digest.py --dump CONFIG      one line per buffer / op with every slot (diff two trees as text)
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


def build(name):
    """The PlanBuilder of configuration `name`, emitted and not yet finalized.  The plan switches are read from the
    environment while this runs and while finalize() runs: the caller sets them (see switches())."""
    from litehandnet_amd import get_model, litehourglass
    from litehandnet_amd.config import litehandnet_cfg
    from litehandnet_amd.plan import PlanBuilder
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
    saved = {s: os.environ.get(s) for s in SWITCHES + ("LHN_INFER_FUSE",)}
    try:
        for s in saved:
            os.environ.pop(s, None)
        for s in CONFIGS[name]["off"]:
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


def record(name):
    with switches(name):
        return digest(build(name))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--write", metavar="FILE")
    ap.add_argument("--dump", metavar="CONFIG", choices=sorted(CONFIGS))
    ap.add_argument("--generated-at", default="", help="commit whose plan.py produced the records (stored in the file)")
    a = ap.parse_args()
    if a.dump:
        with switches(a.dump):
            dump(build(a.dump))
    if a.write:
        doc = {"generated_at": a.generated_at, "configs": {name: record(name) for name in CONFIGS}}
        with open(a.write, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
