"""Inference latency: eval-mode train form vs deployed (re-parameterised) form, each with the inference fusion pass off and on
(plan.set_infer_fuse; LHN_INFER_FUSE in the environment is overridden here).
python scripts/bench_infer.py [A|B|M] [bs] [all|off|on]      (off / on: only the unfused / fused lines, for alternating A/B runs)
Launches: kernel launches of one steady-state forward (tables current), and the table-only launches a first forward adds."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from litehandnet_amd import get_model, plan
from litehandnet_amd.config import litehandnet_cfg

variant = sys.argv[1] if len(sys.argv) > 1 else "B"
bs = int(sys.argv[2]) if len(sys.argv) > 2 else 64
which = sys.argv[3] if len(sys.argv) > 3 else "all"
m = get_model(litehandnet_cfg(variant)).cuda().eval()
x = torch.randn(bs, 3, 256, 256, device="cuda")


side = torch.cuda.Stream()


def launches(fuse):
    p = next(p for k, p in m.__dict__["_engine"].plans.items() if k[0] == tuple(x.shape) and k[-1] == fuse)
    ops = p._keep[1]
    convs = (plan.STEM, plan.PW, plan.DW, plan.KXK)
    tables = sum(o.kind in (plan.TABLE_FILL, plan.FINALIZE) or (o.kind in convs and o.p[2] >= 0) for o in ops)
    steady = sum(o.kind not in (plan.TABLE_FILL, plan.FINALIZE, plan.MEMSET) for o in ops)
    # algorithmic bytes per image of THIS plan's graph: 4 B x (input + output elements) of every convolution launch
    mb = sum(4 * (r["x"].H * r["x"].W * r["x"].C + r["out"].H * r["out"].W * r["out"].C)
             for r in p.pb.recs if r["op"] in convs + (plan.PWDW,)) / 1e6
    return steady, tables, p.pb.n_fused, mb


def timeit(tag, fuse):
    if which != "all" and (which == "on") != fuse:
        return
    plan.set_infer_fuse(fuse)
    with torch.no_grad(), torch.cuda.stream(side):
        for _ in range(5):
            m(x)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(20):
            m(x)
        e1.record()
        torch.cuda.synchronize()
        steady, tables, fused, mb = launches(fuse)
        ms = e0.elapsed_time(e1) / 20
        print(f"{variant} bs{bs} {tag}: {e0.elapsed_time(e1) / 20:.3f} ms/fwd (wall {(time.perf_counter() - t0) * 50:.3f}) "
              f"-> {bs / (e0.elapsed_time(e1) / 20) * 1e3:.0f} img/s; {steady} launches (+{tables} table launches on a first run), "
              f"{fused} fused pairs; {mb:.2f} MB/image of convolution traffic = {mb * bs / ms / 1e3:.3f} TB/s = "
              f"{mb * bs / ms / 1e3 / 8:.3f} of 8 TB/s", flush=True)


timeit("eval (BN running stats)", False)
timeit("eval fused", True)
m.deploy_model()
timeit("deployed", False)
timeit("deployed fused", True)
