"""Inference latency: eval-mode train form vs deployed (re-parameterised) form, each with the inference fusion passes off and on
(plan.set_infer_fuse, plan.set_infer_fuse_dwpw, plan.set_infer_fuse_msrb, plan.set_infer_fuse_bneck, plan.set_infer_fuse_stem) and with the
dense 3x3 convolutions on the split-bf16 MFMA (plan.set_infer_bf16x3), and Lite-HRNet with its channel-weighting blocks as grouped
launches (plan.set_infer_fuse_ccw); LHN_INFER_FUSE / LHN_INFER_FUSE_DWPW / LHN_INFER_FUSE_MSRB / LHN_INFER_FUSE_BNECK / LHN_INFER_FUSE_STEM /
LHN_INFER_BF16X3 / LHN_INFER_FUSE_CCW in the environment are overridden here.
python scripts/bench_infer.py [A|B|M|H|L] [bs] [every|off|on|dwpw|both|msrb|all|bneck|full|bf16x3|bneck+bf16x3|full+bf16x3|stem|full+stem|ccw|full+ccw] [reduction] [channels]
  off / on / dwpw / both / msrb / all / bneck / full: only the lines of that setting (no fusion / 1x1 -> depthwise / depthwise -> 1x1 /
  those two passes / MSRB rounds / those three passes / BottleNecks / all four passes), for alternating runs in fresh processes; every
  (the default): off and on, dwpw and both where the depthwise -> 1x1 pass finds pairs, msrb and all where the MSRB pass finds rounds,
  bneck and full where the BottleNeck pass finds blocks, bf16x3 and full+bf16x3 (the 3x3 pass alone / on top of the four fusion passes)
  where the model has eligible 3x3 convolutions, stem and full+stem (the stem pass alone / on top of the four fusion passes; `full` keeps
  its meaning) where the stem pass finds its pattern (A, M).  A model without a deployed form (H) runs its eval form only.  reduction: the `reduction` of variant A's Residual blocks (config default 4).
  channels: the model width (`input_channel`, config default 128; the reference's width-256 configs run 256).  Every variant runs at 256: the
  256 -> 256 dense 3x3 of variant A's / mynet's Residuals is lhn_conv_kxk_fwd's K-sliced instance (`A 64 off|bneck|full 2 256` is the
  width-256 model itself; scripts/bench_bottleneck256.py times its BottleNecks on their own).  bneck+bf16x3 (only when asked for): the BottleNeck pass and the 3x3 pass together -- the inner 3x3s belong to the
  BottleNeck launches and stay fp32.  LHN_BENCH_BNECK_CHANNELS="128:32,128:64" restricts the BottleNeck pass to those (C, Cm) classes.
Launches: kernel launches of one steady-state forward (tables current), and the table-only launches a first forward adds."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from litehandnet_amd import get_model, plan
from litehandnet_amd.config import litehandnet_cfg

# (infer_fuse, infer_fuse_dwpw, infer_fuse_msrb, infer_fuse_bneck, infer_bf16x3, infer_fuse_stem[, infer_fuse_ccw])
SETTINGS = {"ccw": (False, False, False, False, False, False, True), "full+ccw": (True, True, True, True, False, False, True),
            "off": (False, False, False, False, False, False), "on": (True, False, False, False, False, False),
            "dwpw": (False, True, False, False, False, False), "both": (True, True, False, False, False, False),
            "msrb": (False, False, True, False, False, False), "all": (True, True, True, False, False, False),
            "bneck": (False, False, False, True, False, False), "full": (True, True, True, True, False, False),
            "bf16x3": (False, False, False, False, True, False), "bneck+bf16x3": (False, False, False, True, True, False), "full+bf16x3": (True, True, True, True, True, False),
            "stem": (False, False, False, False, False, True), "full+stem": (True, True, True, True, False, True)}
variant = sys.argv[1] if len(sys.argv) > 1 else "B"
bs = int(sys.argv[2]) if len(sys.argv) > 2 else 64
which = sys.argv[3] if len(sys.argv) > 3 else "every"
assert which == "every" or which in SETTINGS, which
cfg_kw = {"reduction": int(sys.argv[4])} if len(sys.argv) > 4 else {}
if len(sys.argv) > 5:
    cfg_kw["channels"] = int(sys.argv[5])
if os.environ.get("LHN_BENCH_BNECK_CHANNELS"):
    plan.PlanBuilder.FUSE_BNECK_CHANNELS = tuple(tuple(int(v) for v in pair.split(":")) for pair in os.environ["LHN_BENCH_BNECK_CHANNELS"].split(","))
if os.environ.get("LHN_BENCH_CCW_BRANCHES"):
    plan.PlanBuilder.FUSE_CCW_BRANCHES = tuple(int(v) for v in os.environ["LHN_BENCH_CCW_BRANCHES"].split(","))
m = get_model(litehandnet_cfg(variant, **cfg_kw)).cuda().eval()
x = torch.randn(bs, 3, 256, 256, device="cuda")


side = torch.cuda.Stream()


def launches(fuse, dwpw, msrb, bneck, bf16x3, stem, ccw=False):
    p = next(p for k, p in m.__dict__["_engine"].plans.items()
             if k[0] == tuple(x.shape) and k[-1] == fuse and k[-2] == dwpw and k[-3] == msrb and k[-4] == bneck and k[-5] == bf16x3 and k[-6] == stem
             and k[-7] == ccw)
    ops = p._keep[1]
    convs = (plan.STEM, plan.PW, plan.DW, plan.KXK)
    tables = sum(o.kind in (plan.TABLE_FILL, plan.FINALIZE) or (o.kind in convs and o.p[2] >= 0) for o in ops)
    steady = sum(o.kind not in (plan.TABLE_FILL, plan.FINALIZE, plan.MEMSET, plan.CCW_ARG) for o in ops)      # (a CCW_ARG op describes a branch: no launch)
    steady += sum(o.kind == plan.MSRB and o.ws[0] >= 0 for o in ops)       # a pooling MSRB round is two launches: the pass and its fold
    # algorithmic bytes per image of THIS plan's graph: 4 B x (input + output elements) of every convolution launch
    mb = sum(4 * (r["x"].H * r["x"].W * r["x"].C + r["out"].H * r["out"].W * r["out"].C)
             for r in p.pb.recs if r["op"] in convs + (plan.PWDW, plan.DWPW, plan.BNECK, plan.STEMTAIL)) / 1e6
    mb += sum(8 * r["out"].H * r["out"].W * r["out"].C for r in p.pb.recs if r["op"] == plan.MSRB) / 1e6
    mb += sum(8 * t.H * t.W * t.C for r in p.pb.recs if r["op"] == plan.CCW_DW for t in r["ys"]) / 1e6
    return steady, tables, p.pb.n_fused, p.pb.n_fused_dwpw, p.pb.n_fused_msrb, p.pb.n_fused_bneck, mb, p.pb.n_bf16x3, p.pb.n_fused_stem, p.pb.n_fused_ccw


def timeit(form, setting):
    fuse, dwpw, msrb, bneck, bf16x3, stem, ccw = (SETTINGS[setting] + (False,))[:7]
    plan.set_infer_fuse_ccw(ccw)
    plan.set_infer_fuse(fuse)
    plan.set_infer_fuse_dwpw(dwpw)
    plan.set_infer_fuse_msrb(msrb)
    plan.set_infer_fuse_bneck(bneck)
    plan.set_infer_bf16x3(bf16x3)
    plan.set_infer_fuse_stem(stem)
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
        steady, tables, fused, fused_dwpw, fused_msrb, fused_bneck, mb, n_bf16x3, fused_stem, fused_ccw = launches(fuse, dwpw, msrb, bneck, bf16x3, stem, ccw)
        ms = e0.elapsed_time(e1) / 20
        print(f"{variant}{''.join(f' {k[0]}{v}' for k, v in cfg_kw.items())} bs{bs} {form} [{setting}]: {ms:.3f} ms/fwd (wall {(time.perf_counter() - t0) * 50:.3f}) "
              f"-> {bs / ms * 1e3:.0f} img/s; {steady} launches (+{tables} table launches on a first run), "
              f"{fused} 1x1->dw + {fused_dwpw} dw->1x1 fused pairs, {fused_msrb} MSRB rounds, {fused_bneck} BottleNecks, {fused_stem} stems, {fused_ccw} channel-weighting blocks (n_fused_ccw), {n_bf16x3} 3x3 on bf16x3; {mb:.2f} MB/image of convolution traffic = {mb * bs / ms / 1e3:.3f} TB/s = "
              f"{mb * bs / ms / 1e3 / 8:.3f} of 8 TB/s", flush=True)
    return fused_dwpw, fused_msrb, fused_bneck, n_bf16x3, fused_stem, fused_ccw


def form(name):
    if which != "every":
        timeit(name, which)
        return
    timeit(name, "off")
    timeit(name, "on")
    if timeit(name, "dwpw")[0]:
        timeit(name, "both")
    if timeit(name, "msrb")[1]:
        timeit(name, "all")
    if timeit(name, "bneck")[2]:
        timeit(name, "full")
    if timeit(name, "bf16x3")[3]:
        timeit(name, "full+bf16x3")
    if timeit(name, "stem")[4]:
        timeit(name, "full+stem")
    if timeit(name, "ccw")[5]:
        timeit(name, "full+ccw")


form("eval")
if hasattr(m, "deploy_model"):
    m.deploy_model()
    form("deployed")
