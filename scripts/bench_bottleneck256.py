"""The BottleNecks of a variant-A forward at width 256, timed on their own: the network of tests/test_infer_fuse_bneck256_gpu.py
(Hourglass256: the model's thirteen 256-channel BottleNecks on the maps the model gives them, joined by max pools, nearest upsampling
and residual sums) on a [bs, 256, 64, 64] input -- at a 256 x 256 image that is one block on the 64 x 64 map, two at 32 x 32, four at
16 x 16 and six at 8 x 8.  (Written when variant A could not run at this width; `scripts/bench_infer.py A 64 off|bneck|full 2 256` now
times the model itself, this script the BottleNecks without the rest.)
python scripts/bench_bottleneck256.py [bs] [off|bneck|bf16x3|bneck+bf16x3] [reduction]
LHN_BENCH_BNECK_CHANNELS="256:64" restricts the pass to those (C, Cm) classes, as in scripts/bench_infer.py.  Events on the launch
stream, 20 forwards after 5, tables current; the time includes the engine's NCHW <-> NHWC copies of the 268 MB input and output, the
same in every setting."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch
from litehandnet_amd import plan
from test_infer_fuse_bneck256_gpu import Hourglass256

SETTINGS = {"off": (False, False), "bneck": (True, False), "bf16x3": (False, True), "bneck+bf16x3": (True, True)}
bs = int(sys.argv[1]) if len(sys.argv) > 1 else 64
which = sys.argv[2] if len(sys.argv) > 2 else "off"
reduction = int(sys.argv[3]) if len(sys.argv) > 3 else 4
if os.environ.get("LHN_BENCH_BNECK_CHANNELS"):
    plan.PlanBuilder.FUSE_BNECK_CHANNELS = tuple(tuple(int(v) for v in pair.split(":")) for pair in os.environ["LHN_BENCH_BNECK_CHANNELS"].split(","))
for f in (plan.set_infer_fuse, plan.set_infer_fuse_dwpw, plan.set_infer_fuse_msrb, plan.set_infer_fuse_stem, plan.set_infer_fuse_ccw):
    f(False)
plan.set_infer_fuse_bneck(SETTINGS[which][0])
plan.set_infer_bf16x3(SETTINGS[which][1])
torch.manual_seed(0)
m = Hourglass256(reduction).cuda().eval()
x = torch.randn(bs, 256, 64, 64, device="cuda")
side = torch.cuda.Stream()


def timeit(form):
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
        p, = m.__dict__["_engine"].plans.values()
        ops = p._keep[1]
        steady = sum(o.kind not in (plan.TABLE_FILL, plan.FINALIZE, plan.MEMSET) for o in ops)
        classes = sorted((r["x"].C, r["mids"][0].C, r["x"].H) for r in p.pb.recs if r["op"] == plan.BNECK)
        print(f"bnecks256 r{reduction} bs{bs} {form} [{which}]: {e0.elapsed_time(e1) / 20:.3f} ms/fwd (wall {(time.perf_counter() - t0) * 50:.3f}); "
              f"{steady} launches, {p.pb.n_fused_bneck} BottleNecks {sorted(set(c[:2] for c in classes))}, {p.pb.n_bf16x3} 3x3 on bf16x3", flush=True)


timeit("eval")
m.deploy_model()
timeit("deployed")
