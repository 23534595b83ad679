"""Cases of the `mynet` attention MLP (lhn_att_mlp_fwd / lhn_att_mlp_bwd: k_att1 + k_att2, k_att_bwd2 + k_att_bwd1) and of the
squeeze-and-excitation gate MLP (lhn_se_mlp_fwd2 / lhn_se_mlp_bwd2 and their mode-0 wrappers: k_se_fwd, k_se_bwd) run through the C
ABI, with a plain torch reference on the CPU: float64, or float32 to measure what the operation itself loses in the kernels' own
precision.  The forward reference is torch's own batch_norm / conv2d / linear, the backward reference is autograd of that forward under
sum(gate * dgate): neither restates the kernels' formulas.  Imported by tests/test_att_se_gpu.py; run as a script:
    python tests/att_se_cases.py --check-reference        (CPU only: every case's inputs and both references)
    python tests/att_se_cases.py OUT.npz REPEATS NAME ... (a child process with its own environment, e.g. LHN_DETERMINISTIC=1, writes
                                                           every output of the named cases; NAME@wrapper: through lhn_se_mlp_fwd / _bwd)

What each case reaches.  k_att1 / k_att_bwd1: one workgroup per 32 channels, thread = (channel lane, sample lane), 32 sample lanes.
    att_n1_c2_nob3         b3 = db3 = NULL; one live sample lane; two channels of one block; statistics over 9 values
    att_n5_c34             partial second channel block (2 of 32 channels); more sample lanes than samples
    att_n33_c64_mask       second trip of the sample-lane loop, one lane of 32 filled; dropout mask (0 or 1 / 0.7)
    att_n70_c16_mask_pre   third trip; half a channel block; parameter gradients accumulate onto non-zero values; 12 x 12 map
    att_n3_c256_view_pre   largest C: two trips of k_att2's 128 threads, 65,536 dwl addresses; uneven overlapping bins of a 7 x 5 map
                           (all 25 segments distinct); gate and dpool at channel offset 8 of rows 272 wide
    att_n4_c128_hw2x3      the smallest map the segment layout allows (bins of one and two pixels)
    att_n64_c128_mask      the only C the models use, at a model's batch and map size
    att_eval_c64, att_n1_c128_eval   eval mode: running statistics, which keep their bits with num_batches_tracked; forward only
    att_stage12_c64        stage 1 then stage 2 (count_scale = pgrad_scale = 1): must give the bits of att_stage0_c64 (same inputs)
    att_sync2_c48          SyncBatchNorm over two ranks of 3 samples: stage 1 per rank, the gsum vectors added on the host, stage 2
                           with count_scale = 2 (backward: pgrad_scale = 0.5) -- against ONE reference on the concatenated batch
k_se_fwd / k_se_bwd: one workgroup per sample.
    se_n2_c16_j1                      mode 0, one hidden neuron
    se_n5_c40_j2_m1, se_n1_c80_j5_m1  mode 1 (sigmoid(relu(.)) after both layers, the `g > 0.5` derivative rule), Lite-HRNet's C / 16
    se_n70_c20_j1_m1                  mode 1, C below a wave, many samples
    se_n3_c256_j64_view_pre           both limits of the API; inv_hw = 1 / 35; the view and pre-filled gradients as above
    se_n3_c256_j16_m1                 mode 1 at the largest C
    se_n33_c128_j8_nobias             b1 = b2 = db1 = db2 = NULL; non-square 8 x 6 map
    se_n64_c128_j8_pre (+ _m1)        the largest N x C of the models, both modes
    se_zero_preact (+ _m1)            a hidden pre-activation of exactly zero: relu'(0) = 0 (see _gen_se)

Inputs keep every branch decision away from its kink: a reference whose float32 form flips one ReLU would widen the bar and hide a
failure.  att: plain normal `pooled` cannot keep 9 N C BatchNorm outputs off zero, a bimodal draw 0.25 * sign * (1 + 0.5 |z|) can;
SE: biases of +-3 (alternating) under pre-activations of unit scale.  A seed at which a condition fails is passed over (ten seeds);
`--check-reference` asserts the conditions for the seed found and fails for a case without one."""
import ctypes as C
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ca_mlp_cases import EPS, FLOOR, MARGIN, MOMENTUM, PAD, PREFILL, SLOTS, _alloc, _bins, _dpool25, _outside, _rand, rel_err  # noqa: E402,F401
from litehandnet_amd import _lib  # noqa: E402

# hw: the gated map (bin sizes of the pooled gradient);  mask: dropout mask;  pre: parameter gradients start non-zero;
# coff / cs: the gate covers channels [coff, coff + c) of a buffer cs wide;  staged: stage 1 then stage 2 on one rank;  ranks: SyncBatchNorm
ATT = {
    "att_n1_c2_nob3": dict(n=1, c=2, hw=(6, 6), nob3=True),
    "att_n5_c34": dict(n=5, c=34, hw=(6, 6)),
    "att_n33_c64_mask": dict(n=33, c=64, hw=(6, 6), mask=True),
    "att_n70_c16_mask_pre": dict(n=70, c=16, hw=(12, 12), mask=True, pre=True),
    "att_n3_c256_view_pre": dict(n=3, c=256, hw=(7, 5), coff=8, cs=256 + 16, pre=True),
    "att_n4_c128_hw2x3": dict(n=4, c=128, hw=(2, 3)),
    "att_n64_c128_mask": dict(n=64, c=128, hw=(8, 8), mask=True),
    "att_eval_c64": dict(n=4, c=64, hw=(6, 6), mode="eval"),
    "att_n1_c128_eval": dict(n=1, c=128, hw=(6, 6), mode="eval"),
    "att_stage12_c64": dict(n=6, c=64, hw=(6, 6), mask=True, staged=True),
    "att_stage0_c64": dict(n=6, c=64, hw=(6, 6), mask=True, like="att_stage12_c64"),
    "att_sync2_c48": dict(n=6, c=48, hw=(6, 6), mask=True, ranks=2),
}
# m: mode (0 SEBlock, 1 SpatialWeighting);  nobias: the NULL-bias pair;  zero: the directed case of _gen_se
SE = {
    "se_n2_c16_j1": dict(n=2, c=16, j=1, m=0, hw=(4, 4)),
    "se_n5_c40_j2_m1": dict(n=5, c=40, j=2, m=1, hw=(8, 8)),
    "se_n1_c80_j5_m1": dict(n=1, c=80, j=5, m=1, hw=(8, 8)),
    "se_n70_c20_j1_m1": dict(n=70, c=20, j=1, m=1, hw=(6, 6)),
    "se_n3_c256_j64_view_pre": dict(n=3, c=256, j=64, m=0, hw=(7, 5), coff=8, cs=256 + 16, pre=True),
    "se_n3_c256_j16_m1": dict(n=3, c=256, j=16, m=1, hw=(8, 8)),
    "se_n33_c128_j8_nobias": dict(n=33, c=128, j=8, m=0, hw=(8, 6), nobias=True),
    "se_n64_c128_j8_pre": dict(n=64, c=128, j=8, m=0, hw=(8, 8), pre=True),
    "se_n64_c128_j8_pre_m1": dict(n=64, c=128, j=8, m=1, hw=(8, 8), pre=True),
    "se_zero_preact": dict(n=2, c=16, j=2, m=0, hw=(4, 4), zero=True),
    "se_zero_preact_m1": dict(n=2, c=16, j=2, m=1, hw=(4, 4), zero=True),
}
CASES = dict(ATT, **SE)
ATT_GRADS = ("dgamma", "dbeta", "dw3", "db3", "dwl", "dbl")
SE_GRADS = ("dw1", "db1", "dw2", "db2")
# Outputs the kernels accumulate with float atomics over the samples' workgroups (k_att_bwd2: dbl, dwl; k_se_bwd: db2, dw2, db1, dw1):
# their last bits depend on the order of arrival unless LHN_DETERMINISTIC=1 runs the one ordered workgroup.  Everything else --
# the whole forward, dad (one writer per element), and what k_att_bwd1 derives from it with one writer per channel: dpool, dgamma,
# dbeta, dw3, db3; k_se_bwd's dpool -- is written without atomics and repeats its bits in every mode.
ATOMIC = ("dwl", "dbl", "dw1", "db1", "dw2", "db2")


def mode(name):
    return CASES[name].get("mode", "train")


def has_bwd(name):
    return mode(name) == "train"


def _alt(k, amp, seed):
    """+amp, -amp, +amp, ... plus noise of scale 0.2"""
    return amp * torch.tensor([1.0 if i % 2 == 0 else -1.0 for i in range(k)]) + 0.2 * _rand((k,), seed)


def _gen_att(c, seed):
    n, ch = c["n"], c["c"]
    g = {"seed": seed}
    sign = torch.from_numpy(np.random.Generator(np.random.PCG64(seed + 30)).random((n, 9, ch)) < 0.5).float() * 2 - 1
    g["pooled"] = 0.25 * sign * (1 + 0.5 * _rand((n, 9, ch), seed).abs())
    g["gamma"] = 1 + 0.3 * _rand((ch,), seed + 1)
    g["beta"] = 0.2 * _rand((ch,), seed + 2)
    g["rmean"] = 0.05 * _rand((ch,), seed + 3)
    g["rvar"] = 0.05 + 0.02 * _rand((ch,), seed + 4).abs()
    g["w3"] = _rand((ch, 9), seed + 5, 1.0 / 3.0)
    if not c.get("nob3"):
        g["b3"] = 0.3 * _rand((ch,), seed + 6)
    g["wl"] = _rand((ch, ch), seed + 7, ch ** -0.5)
    g["bl"] = 0.3 * _rand((ch,), seed + 8)
    if c.get("mask"):          # Dropout(p = 0.3) on the [N, C] tensor: 0 or 1 / 0.7
        g["mask"] = torch.from_numpy(np.random.Generator(np.random.PCG64(seed + 10)).random((n, ch)) >= 0.3).float() / 0.7
    g["dgate"] = _rand((n, ch), seed + 11)
    for i, k in enumerate(ATT_GRADS):
        shp = {"dw3": (ch, 9), "dwl": (ch, ch)}.get(k, (ch,))
        if k != "db3" or "b3" in g:
            g[k + "_0"] = 0.05 * _rand(shp, seed + 20 + i) if c.get("pre") else torch.zeros(shp)
    return g


def _gen_se(c, seed):
    """Pre-activations of unit scale under biases of +-3.  One hidden neuron has no alternating bias: it draws a plain one and the
    seed search sees to it that both ReLU branches are taken; so does the NULL-bias case.
    zero (exempt from the MARGIN condition by design, in its one entry): sample 0 has pooled = 0 and b1 = (0, -3), so its hidden
    pre-activations are exactly 0 and -3: both units dead, and unit 1 is dead for sample 1 as well.  torch's relu'(0) = 0 is the rule
    the kernel's `sh > 0` (mode 0) and `sh > 0.5` (mode 1: sigmoid(0) = 0.5 exactly) tests must match."""
    n, ch, j, m = c["n"], c["c"], c["j"], c["m"]
    g = {"seed": seed}
    g["pooled"] = _rand((n, ch), seed, 0.5)
    g["w1"] = _rand((j, ch), seed + 1, 2.0 * ch ** -0.5)
    g["w2"] = _rand((ch, j), seed + 2, 0.5 * j ** -0.5)
    if not c.get("nobias"):
        g["b1"] = _alt(j, 3.0, seed + 3) if j > 1 else 0.3 * _rand((j,), seed + 3)
        g["b2"] = _alt(ch, 3.0, seed + 4) if m == 1 else 0.3 * _rand((ch,), seed + 4)
    if c.get("zero"):
        g["pooled"][0] = 0
        g["b1"] = torch.tensor([0.0, -3.0])
    g["dgate"] = _rand((n, ch), seed + 11)
    for i, k in enumerate(SE_GRADS):
        shp = {"dw1": (j, ch), "db1": (j,), "dw2": (ch, j), "db2": (ch,)}[k]
        if "b1" in g or k in ("dw1", "dw2"):
            g[k + "_0"] = 0.05 * _rand(shp, seed + 20 + i) if c.get("pre") else torch.zeros(shp)
    return g


def _cast(g, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) else v) for k, v in g.items()}


# ---------------------------------------------------------------- reference
def _att_forward(t, train):
    """sigmoid(Linear(dropout(dw3x3_valid(relu(BatchNorm2d(pooled))) + b3))) on the pooled [N, 9, C] tensor (a 3 x 3 map per channel)."""
    p = t["pooled"]
    n, _, ch = p.shape
    rm, rv = t["rmean"].clone(), t["rvar"].clone()
    u = F.batch_norm(p.permute(0, 2, 1).reshape(n, ch, 3, 3), rm, rv, t["gamma"], t["beta"], train, MOMENTUM, EPS)
    a = F.conv2d(torch.relu(u), t["w3"].view(ch, 1, 3, 3), t.get("b3"), groups=ch).view(n, ch)
    ad = a * t["mask"] if "mask" in t else a
    g = torch.sigmoid(F.linear(ad, t["wl"], t["bl"]))
    if train:
        mean, var = p.detach().mean((0, 1)), p.detach().var((0, 1), unbiased=False)
    else:
        mean, var = t["rmean"], t["rvar"]
    return dict(u=u, ad=ad, g=g, gate=g, mean=mean, invstd=1.0 / torch.sqrt(var + EPS), rmean=rm, rvar=rv)


def _se_forward(t, m):
    """mode 0: sigmoid(up(relu(down(pooled)))); mode 1: sigmoid(relu(.)) after both layers."""
    pre = F.linear(t["pooled"], t["w1"], t.get("b1"))
    h = torch.relu(pre)
    if m == 1:
        h = torch.sigmoid(h)
    z = F.linear(h, t["w2"], t.get("b2"))
    g = torch.sigmoid(torch.relu(z) if m == 1 else z)
    return dict(pre=pre, h=h, z=z, g=g, gate=g)


def _np(out):
    return {k: v.detach().double().numpy() for k, v in out.items()}


def _att_reference(name, t, dtype):
    c = ATT[name]
    train, ranks = has_bwd(name), c.get("ranks", 1)
    params = [k for k in ("gamma", "beta", "w3", "b3", "wl", "bl") if k in t]
    if train:
        for k in ["pooled"] + params:
            t[k] = t[k].clone().requires_grad_()
    f = _att_forward(t, train)
    full = {k: f[k] for k in ("gate", "ad", "g", "mean", "invstd", "rmean", "rvar")}
    if train:
        gr = torch.autograd.grad((f["g"] * t["dgate"]).sum(), [t["pooled"], f["ad"]] + [t[k] for k in params], retain_graph=True)
        binv = torch.tensor([1.0 / ((bh[1] - bh[0]) * (bw[1] - bw[0])) for bh in _bins(c["hw"][0]) for bw in _bins(c["hw"][1])], dtype=dtype)
        full["dpool"], full["dad"] = _dpool25(gr[0] * binv[None, :, None]), gr[1]
        pg = dict(zip(params, gr[2:]))
    if ranks == 1:
        if train:
            for k in params:
                full["d" + k] = t["d" + k + "_0"] + pg[k]
        return _np(full)
    # SyncBatchNorm: every rank holds its rows of the batch's result; d(gamma), d(beta) come from the global sums scaled by 1 / ranks;
    # the convolution's and the Linear's gradients are the rank's own (no cross-sample term after the BatchNorm): a backward of the
    # same graph with the other ranks' dgate set to zero
    out, nr = {}, c["n"] // ranks
    for r in range(ranks):
        rows = slice(r * nr, (r + 1) * nr)
        for k, v in full.items():
            out[f"r{r}_{k}"] = v[rows] if k in ("gate", "ad", "g", "dpool", "dad") else v
        dg = torch.zeros_like(t["dgate"])
        dg[rows] = t["dgate"][rows]
        own = dict(zip(params, torch.autograd.grad((f["g"] * dg).sum(), [t[k] for k in params], retain_graph=True)))
        for k in params:
            out[f"r{r}_d{k}"] = t["d" + k + "_0"] + (pg[k] / ranks if k in ("gamma", "beta") else own[k])
    return _np(out)


def _se_reference(name, t, dtype):
    c = SE[name]
    params = [k for k in ("w1", "b1", "w2", "b2") if k in t]
    for k in ["pooled"] + params:
        t[k] = t[k].clone().requires_grad_()
    f = _se_forward(t, c["m"])
    out = {k: f[k] for k in ("gate", "h", "g")}
    gr = torch.autograd.grad((f["g"] * t["dgate"]).sum(), [t["pooled"]] + [t[k] for k in params])
    out["dpool"] = (gr[0] / (c["hw"][0] * c["hw"][1]))[:, None, :].expand(c["n"], SLOTS, c["c"])      # one global bin: every slot
    for k, v in zip(params, gr[1:]):
        out["d" + k] = t["d" + k + "_0"] + v
    return _np(out)


def reference(name, g=None, dtype=torch.float64):
    """Every output as numpy float64 arrays, computed in `dtype`."""
    t = _cast(g or inputs(name), dtype)
    return _att_reference(name, t, dtype) if name in ATT else _se_reference(name, t, dtype)


def decisions(name, g, dtype=torch.float64):
    """[(what, pre-activations whose sign a kernel branches on)], computed in `dtype`; the exact zero of the directed case left out."""
    t = _cast(g, dtype)
    if name in ATT:
        return [("BatchNorm output", _att_forward(t, has_bwd(name))["u"].detach().reshape(-1))]
    f, c = _se_forward(t, SE[name]["m"]), SE[name]
    pre = f["pre"].detach().reshape(-1)
    res = [("hidden pre-activation", pre[1:] if c.get("zero") else pre)]
    if c["m"] == 1:
        res.append(("output pre-activation", f["z"].detach().reshape(-1)))
    return res


def conditions(name, g):
    """What keeps `g` from being a valid input of the case ([] = nothing)."""
    bad = []
    for (what, d64), (_, d32) in zip(decisions(name, g), decisions(name, g, torch.float32)):
        if float(d64.abs().min()) < MARGIN:
            bad.append(f"a {what} within {MARGIN} of zero")
        if not torch.equal(d64 > 0, d32 > 0):
            bad.append(f"float32 and float64 disagree about the branch of a {what}")
        if not (bool((d64 > 0).any()) and bool((d64 < 0).any())):
            bad.append(f"one branch of the {what}s is never taken")
    if name in SE and SE[name].get("zero"):
        pre = _se_forward(_cast(g, torch.float64), SE[name]["m"])["pre"]
        if not (float(pre[0, 0]) == 0.0 and float(pre[0, 1]) < -MARGIN and float(pre[1, 0]) > MARGIN and float(pre[1, 1]) < -MARGIN):
            bad.append("the directed pre-activations are not (0, < 0) for sample 0 and (> 0, < 0) for sample 1")
    return bad


_INPUTS = {}


def inputs(name, seed=7):
    """Seeded inputs; a seed at which a branch condition fails is passed over (seed, seed + 100, ...: ten of them)."""
    name = CASES[name].get("like", name)
    if (name, seed) not in _INPUTS:
        why = []
        for s in range(seed, seed + 1000, 100):
            g = _gen_att(ATT[name], s) if name in ATT else _gen_se(SE[name], s)
            bad = conditions(name, g)
            if not bad:
                _INPUTS[(name, seed)] = g
                break
            why.append(f"{s}: {bad[0]}")
        else:
            raise AssertionError(f"{name}: no seed meets the input conditions ({'; '.join(why)})")
    return _INPUTS[(name, seed)]


def dead_parts(name, out):
    """The directed case: what flows through a dead hidden unit, as arrays that must be exact zeros (`out`: kernel or reference)."""
    m = SE[name]["m"]
    parts = {"dpool[0]": out["dpool"][0], "dw1[1]": out["dw1"][1], "db1[1]": out["db1"][1:2],
             "h[0] - relu(0)": out["h"][0] - (0.5 if m else 0.0), "h[:, 1] - relu(<0)": out["h"][:, 1] - (0.5 if m else 0.0)}
    if m == 0:
        parts["dw2[:, 1]"] = out["dw2"][:, 1]
    return parts


# ---------------------------------------------------------------- kernels
def _args_att_fwd(k, d, n, ch, cs, coff, train, stage, scale):
    p, fl = _lib.ptr, C.c_float
    return dict(pooled=p(k["pooled"]), gamma=p(d["gamma"]), beta=p(d["beta"]), rmean=p(k["rmean"][1]), rvar=p(k["rvar"][1]), nbt=p(k["nbt"]),
                w3=p(d["w3"]), b3=p(d.get("b3")), wl=p(d["wl"]), bl=p(d["bl"]), dropmask=p(k["mask"]), gate=p(k["gate"][1]), gate_stride=cs,
                gate_coff=coff, save=p(k["save"][1]), N=n, C=ch, eps=fl(EPS), momentum=fl(MOMENTUM), training=train, stage=stage,
                gsum=p(k["gsum"]), count_scale=C.c_double(scale), stream=_lib.stream())


def _args_att_bwd(k, d, n, ch, cs, coff, hw, stage, scale, pscale):
    p = _lib.ptr
    a = dict(pooled=p(k["pooled"]), gamma=p(d["gamma"]), beta=p(d["beta"]), w3=p(d["w3"]), wl=p(d["wl"]), dropmask=p(k["mask"]),
             save=p(k["save"][1]), dgate=p(k["dgate"]), dpool=p(k["dpool"][1]), cstride=cs, coff=coff, H=hw[0], W=hw[1])
    for g in ATT_GRADS:
        a[g] = p(k[g][1] if g in k else None)
    a.update(N=n, C=ch, stage=stage, gsum=p(k["gsumb"]), count_scale=C.c_double(scale), pgrad_scale=C.c_float(pscale), stream=_lib.stream())
    return a


def _att_ctx(c, d, g, dev, rows):
    """The buffers of one rank: every output in front of PAD prefilled elements, `save` at exactly the size include/lhn.h states."""
    n, ch, cs = rows.stop - rows.start, c["c"], c.get("cs", c["c"])
    k = dict(pooled=d["pooled"][rows].contiguous(), mask=d["mask"][rows].contiguous() if "mask" in d else None,
             dgate=d["dgate"][rows].contiguous(), save=_alloc((3 * n * ch + 2 * ch,), dev), gate=_alloc((n, cs), dev),
             rmean=_alloc((ch,), dev, d["rmean"]), rvar=_alloc((ch,), dev, d["rvar"]),
             nbt=torch.full((1 + PAD,), 5, dtype=torch.int64, device=dev), dpool=_alloc((n, SLOTS, cs), dev),
             gsum=torch.full((2 * ch + PAD,), PREFILL, dtype=torch.float64, device=dev),
             gsumb=torch.full((2 * ch + PAD,), PREFILL, dtype=torch.float64, device=dev))
    for q in ATT_GRADS:
        if q + "_0" in g:
            k[q] = _alloc(tuple(g[q + "_0"].shape), dev, g[q + "_0"])
    return k


def _writable(k):
    """Every buffer of a context that a call may write: [(name, flat tensor)]."""
    return [(q, v[0] if isinstance(v, tuple) else v) for q, v in k.items()
            if q not in ("pooled", "mask", "dgate") and v is not None]


def _tail_ok(pair):
    flat, view = pair
    return bool((flat[view.numel():] == PREFILL).all())


def _run_att(name, dev, g):
    c = ATT[name]
    d = {q: (v.to(dev) if torch.is_tensor(v) else v) for q, v in g.items()}
    L = _lib.lib()
    R, ch, cs, coff, train = c.get("ranks", 1), c["c"], c.get("cs", c["c"]), c.get("coff", 0), 1 if has_bwd(name) else 0
    n = c["n"] // R
    ctx = [_att_ctx(c, d, g, dev, slice(r * n, (r + 1) * n)) for r in range(R)]
    nc = n * ch

    def allreduce(key):            # the all-reduce of SyncBatchNorm: float64 on the host, the sum to every rank
        torch.cuda.synchronize()
        tot = sum(k[key][:2 * ch].cpu() for k in ctx)
        for k in ctx:
            k[key][:2 * ch] = tot.to(dev)

    def fwd(stage, scale=1.0):
        for r, k in enumerate(ctx):
            _lib.check(L.lhn_att_mlp_fwd(*_args_att_fwd(k, d, n, ch, cs, coff, train, stage, scale).values()), f"lhn_att_mlp_fwd {name} stage {stage} rank {r}")
    if R > 1 or c.get("staged"):
        fwd(1, float(R))
        torch.cuda.synchronize()
        stage1_ok = all(bool((k["save"][0] == PREFILL).all()) and bool((k["gate"][0] == PREFILL).all()) and int(k["nbt"][0]) == 5 and
                        torch.equal(k["rmean"][1], d["rmean"]) and torch.equal(k["rvar"][1], d["rvar"]) for k in ctx)     # sums only
        if R > 1:
            allreduce("gsum")
        fwd(2, float(R))
    else:
        stage1_ok = True
        fwd(0)
    torch.cuda.synchronize()
    out = {}
    for r, k in enumerate(ctx):
        pf, save, gate = (f"r{r}_" if R > 1 else ""), k["save"][1], k["gate"][1]
        for q, (o, shp) in {"ad": (0, (n, ch)), "g": (nc, (n, ch)), "mean": (2 * nc, (ch,)), "invstd": (2 * nc + ch, (ch,))}.items():
            out[pf + q] = save[o:o + int(np.prod(shp))].view(shp).cpu().numpy()
        out[pf + "gate"] = gate[:, coff:coff + ch].cpu().numpy()
        out[pf + "rmean"], out[pf + "rvar"], out[pf + "nbt"] = k["rmean"][1].cpu().numpy(), k["rvar"][1].cpu().numpy(), k["nbt"][:1].cpu().numpy()
        out[pf + "gate_ok"] = np.array(_tail_ok(k["gate"]) and bool((_outside(gate, coff, ch) == PREFILL).all()))
        out[pf + "stats_ok"] = np.array(_tail_ok(k["rmean"]) and _tail_ok(k["rvar"]) and bool((k["nbt"][1:] == 5).all()) and stage1_ok and
                                        (bool(train) or (torch.equal(k["rmean"][1], d["rmean"]) and torch.equal(k["rvar"][1], d["rvar"]))))
        k["fwd_scratch_ok"] = bool((save[2 * nc + 2 * ch:] == PREFILL).all())            # the forward leaves the dad rows alone
        k["fwd_gsum_ok"] = bool((k["gsumb"] == PREFILL).all()) and bool((k["gsum"][2 * ch:] == PREFILL).all()) and \
            (R > 1 or bool(c.get("staged")) or bool((k["gsum"] == PREFILL).all()))         # stage 0 leaves gsum alone
    if train:
        def bwd(stage, scale=1.0, pscale=1.0):
            for r, k in enumerate(ctx):
                _lib.check(L.lhn_att_mlp_bwd(*_args_att_bwd(k, d, n, ch, cs, coff, c["hw"], stage, scale, pscale).values()),
                           f"lhn_att_mlp_bwd {name} stage {stage} rank {r}")
        if R > 1 or c.get("staged"):
            bwd(1, float(R), 1.0 / R)
            if R > 1:
                allreduce("gsumb")
            bwd(2, float(R), 1.0 / R)
        else:
            bwd(0)
        torch.cuda.synchronize()
    for r, k in enumerate(ctx):
        pf = f"r{r}_" if R > 1 else ""
        if train:
            ok = True
            for q in ATT_GRADS:
                if q in k:
                    out[pf + q] = k[q][1].cpu().numpy()
                    ok = ok and _tail_ok(k[q])
            out[pf + "grads_ok"] = np.array(ok)
            dpool = k["dpool"][1]
            out[pf + "dpool"] = dpool[:, :, coff:coff + ch].cpu().numpy()
            out[pf + "dpool_ok"] = np.array(_tail_ok(k["dpool"]) and bool((_outside(dpool, coff, ch) == PREFILL).all()))
            out[pf + "dad"] = k["save"][1][2 * nc + 2 * ch:].view(n, ch).cpu().numpy()
        else:
            out[pf + "dpool_ok"] = np.array(bool((k["dpool"][0] == PREFILL).all()))
        out[pf + "save_ok"] = np.array(_tail_ok(k["save"]) and k["fwd_scratch_ok"])
        staged = R > 1 or bool(c.get("staged"))
        out[pf + "gsum_ok"] = np.array(k["fwd_gsum_ok"] and bool((k["gsum"][2 * ch:] == PREFILL).all()) and bool((k["gsumb"][2 * ch:] == PREFILL).all()) and
                                       (staged or (bool((k["gsum"] == PREFILL).all()) and bool((k["gsumb"] == PREFILL).all()))))
    return out


def _args_se_fwd(k, d, n, ch, j, cs, coff, m):
    p = _lib.ptr
    return dict(pooled=p(d["pooled"]), w1=p(d["w1"]), b1=p(d.get("b1")), w2=p(d["w2"]), b2=p(d.get("b2")), gate=p(k["gate"][1]), gate_stride=cs,
                gate_coff=coff, save=p(k["save"][1]), N=n, C=ch, J=j, mode=m, stream=_lib.stream())


def _args_se_bwd(k, d, n, ch, j, cs, coff, hw, m):
    p = _lib.ptr
    a = dict(pooled=p(d["pooled"]), w1=p(d["w1"]), w2=p(d["w2"]), save=p(k["save"][1]), dgate=p(d["dgate"]), dpool=p(k["dpool"][1]), cstride=cs,
             coff=coff, H=hw[0], W=hw[1])
    for g in SE_GRADS:
        a[g] = p(k[g][1] if g in k else None)
    a.update(N=n, C=ch, J=j, mode=m, stream=_lib.stream())
    return a


def _se_ctx(c, g, dev):
    n, ch, j, cs = c["n"], c["c"], c["j"], c.get("cs", c["c"])
    k = dict(save=_alloc((n * (j + ch),), dev), gate=_alloc((n, cs), dev), dpool=_alloc((n, SLOTS, cs), dev))
    for q in SE_GRADS:
        if q + "_0" in g:
            k[q] = _alloc(tuple(g[q + "_0"].shape), dev, g[q + "_0"])
    return k


def _without(a, key):
    return [v for q, v in a.items() if q != key]


def _run_se(name, dev, g, wrapper=False):
    c = SE[name]
    d = {q: (v.to(dev) if torch.is_tensor(v) else v) for q, v in g.items()}
    L = _lib.lib()
    n, ch, j, m, cs, coff = c["n"], c["c"], c["j"], c["m"], c.get("cs", c["c"]), c.get("coff", 0)
    k = _se_ctx(c, g, dev)
    a = _args_se_fwd(k, d, n, ch, j, cs, coff, m)
    if wrapper:                      # lhn_se_mlp_fwd / lhn_se_mlp_bwd: the same calls without the mode argument
        assert m == 0
        _lib.check(L.lhn_se_mlp_fwd(*_without(a, "mode")), f"lhn_se_mlp_fwd {name}")
    else:
        _lib.check(L.lhn_se_mlp_fwd2(*a.values()), f"lhn_se_mlp_fwd2 {name}")
    torch.cuda.synchronize()
    save, gate, dpool = k["save"][1], k["gate"][1], k["dpool"][1]
    out = {"h": save[:n * j].view(n, j).cpu().numpy(), "g": save[n * j:].view(n, ch).cpu().numpy(), "gate": gate[:, coff:coff + ch].cpu().numpy()}
    out["gate_ok"] = np.array(_tail_ok(k["gate"]) and bool((_outside(gate, coff, ch) == PREFILL).all()))
    fwd_ok = bool((k["dpool"][0] == PREFILL).all())
    a = _args_se_bwd(k, d, n, ch, j, cs, coff, c["hw"], m)
    if wrapper:
        _lib.check(L.lhn_se_mlp_bwd(*_without(a, "mode")), f"lhn_se_mlp_bwd {name}")
    else:
        _lib.check(L.lhn_se_mlp_bwd2(*a.values()), f"lhn_se_mlp_bwd2 {name}")
    torch.cuda.synchronize()
    ok = True
    for q in SE_GRADS:
        if q in k:
            out[q] = k[q][1].cpu().numpy()
            ok = ok and _tail_ok(k[q])
    out["grads_ok"] = np.array(ok)
    out["dpool"] = dpool[:, :, coff:coff + ch].cpu().numpy()
    out["dpool_ok"] = np.array(fwd_ok and _tail_ok(k["dpool"]) and bool((_outside(dpool, coff, ch) == PREFILL).all()))
    out["save_ok"] = np.array(_tail_ok(k["save"]))
    return out


def run(name, dev, g=None, wrapper=False):
    """Forward, then (training cases) backward; outputs as numpy arrays plus `*_ok` flags: every float outside an output keeps its bits."""
    g = g or inputs(name)
    return _run_att(name, dev, g) if name in ATT else _run_se(name, dev, g, wrapper)


# ---------------------------------------------------------------- refusals
# calls the library must refuse (status 1, the reason in lhn_last_error, nothing launched: every prefilled output keeps its bits).
# name: (entry point, arguments replaced in an otherwise valid call, text lhn_last_error must hold).  The valid calls: att N = 2,
# C = 16, 6 x 6 map, channels [8, 24) of rows 32 wide, b3 and a mask; SE the same with J = 2; ca N = 2, C = 4, whole rows.
NULL = C.c_void_p(0)
REFUSE = {
    "att_fwd_null_wl": ("att_fwd", dict(wl=NULL), "null pointer"),
    "att_fwd_null_save": ("att_fwd", dict(save=NULL), "null pointer"),
    "att_fwd_c0": ("att_fwd", dict(C=0), "lhn_att_mlp_fwd"),
    "att_fwd_c257": ("att_fwd", dict(C=257), "lhn_att_mlp_fwd"),
    "att_fwd_n0": ("att_fwd", dict(N=0), "lhn_att_mlp_fwd"),
    "att_fwd_stage1_nogsum": ("att_fwd", dict(stage=1, gsum=NULL), "needs gsum"),
    "att_fwd_stage3": ("att_fwd", dict(stage=3), "stage 3"),
    "att_fwd_count_half": ("att_fwd", dict(stage=2, count_scale=C.c_double(0.5)), "stage 2"),
    "att_fwd_gate_stride": ("att_fwd", dict(gate_stride=20), "gate_stride"),
    "att_bwd_null_dgate": ("att_bwd", dict(dgate=NULL), "null pointer"),
    "att_bwd_null_dwl": ("att_bwd", dict(dwl=NULL), "null pointer"),
    "att_bwd_c0": ("att_bwd", dict(C=0), "lhn_att_mlp_bwd"),
    "att_bwd_c257": ("att_bwd", dict(C=257), "lhn_att_mlp_bwd"),
    "att_bwd_n0": ("att_bwd", dict(N=0), "lhn_att_mlp_bwd"),
    "att_bwd_stage1_nogsum": ("att_bwd", dict(stage=1, gsum=NULL), "needs gsum"),
    "att_bwd_stage3": ("att_bwd", dict(stage=3), "stage 3"),
    "att_bwd_count_half": ("att_bwd", dict(stage=2, count_scale=C.c_double(0.5)), "stage 2"),
    "att_bwd_h1": ("att_bwd", dict(H=1), "segment layout"),
    "att_bwd_w1": ("att_bwd", dict(W=1), "segment layout"),
    "att_bwd_h0": ("att_bwd", dict(H=0), "segment layout"),
    "att_bwd_cstride": ("att_bwd", dict(cstride=20), "cstride"),
    "se_fwd_null_w2": ("se_fwd", dict(w2=NULL), "null pointer"),
    "se_fwd_c0": ("se_fwd", dict(C=0), "lhn_se_mlp_fwd"),
    "se_fwd_c257": ("se_fwd", dict(C=257), "lhn_se_mlp_fwd"),
    "se_fwd_n0": ("se_fwd", dict(N=0), "lhn_se_mlp_fwd"),
    "se_fwd_j0": ("se_fwd", dict(J=0), "lhn_se_mlp_fwd"),
    "se_fwd_j65": ("se_fwd", dict(J=65), "lhn_se_mlp_fwd"),
    "se_fwd_only_b1": ("se_fwd", dict(b2=NULL), "both or neither"),
    "se_fwd_only_b2": ("se_fwd", dict(b1=NULL), "both or neither"),
    "se_fwd_mode2": ("se_fwd", dict(mode=2), "mode"),
    "se_fwd_gate_stride": ("se_fwd", dict(gate_stride=20), "gate_stride"),
    "se_bwd_null_dpool": ("se_bwd", dict(dpool=NULL), "null pointer"),
    "se_bwd_c0": ("se_bwd", dict(C=0), "lhn_se_mlp_bwd"),
    "se_bwd_c257": ("se_bwd", dict(C=257), "lhn_se_mlp_bwd"),
    "se_bwd_n0": ("se_bwd", dict(N=0), "lhn_se_mlp_bwd"),
    "se_bwd_j0": ("se_bwd", dict(J=0), "lhn_se_mlp_bwd"),
    "se_bwd_j65": ("se_bwd", dict(J=65), "lhn_se_mlp_bwd"),
    "se_bwd_h0": ("se_bwd", dict(H=0), "lhn_se_mlp_bwd"),
    "se_bwd_only_db1": ("se_bwd", dict(db2=NULL), "both or neither"),
    "se_bwd_only_db2": ("se_bwd", dict(db1=NULL), "both or neither"),
    "se_bwd_mode_neg": ("se_bwd", dict(mode=-1), "mode"),
    "se_bwd_cstride": ("se_bwd", dict(cstride=20), "cstride"),
    "ca_bwd_h1": ("ca_bwd", dict(H=1), "segment layout"),
    "ca_bwd_w1": ("ca_bwd", dict(W=1), "segment layout"),
}
_REFUSE_ATT = dict(n=2, c=16, hw=(6, 6), coff=8, cs=32, mask=True)
_REFUSE_SE = dict(n=2, c=16, j=2, m=0, hw=(6, 6), coff=8, cs=32)


def refuse(name, dev):
    """The refused call of REFUSE[name]: (status, every writable buffer kept its bits, lhn_last_error)."""
    kind, over, _ = REFUSE[name]
    L = _lib.lib()
    if kind.startswith("att"):
        c = _REFUSE_ATT
        g = _gen_att(c, 7)
        d = {q: (v.to(dev) if torch.is_tensor(v) else v) for q, v in g.items()}
        k = _att_ctx(c, d, g, dev, slice(0, c["n"]))
        a = _args_att_fwd(k, d, c["n"], c["c"], c["cs"], c["coff"], 1, 0, 1.0) if kind == "att_fwd" else \
            _args_att_bwd(k, d, c["n"], c["c"], c["cs"], c["coff"], c["hw"], 0, 1.0, 1.0)
        fn = L.lhn_att_mlp_fwd if kind == "att_fwd" else L.lhn_att_mlp_bwd
    elif kind.startswith("se"):
        c = _REFUSE_SE
        g = _gen_se(c, 7)
        d = {q: (v.to(dev) if torch.is_tensor(v) else v) for q, v in g.items()}
        k = _se_ctx(c, g, dev)
        a = _args_se_fwd(k, d, c["n"], c["c"], c["j"], c["cs"], c["coff"], 0) if kind == "se_fwd" else \
            _args_se_bwd(k, d, c["n"], c["c"], c["j"], c["cs"], c["coff"], c["hw"], 0)
        fn = L.lhn_se_mlp_fwd2 if kind == "se_fwd" else L.lhn_se_mlp_bwd2
    else:                            # lhn_ca_mlp_bwd2 writes its pooled gradient with the same segment writer
        n, ch, p = 2, 4, _lib.ptr
        d = {q: _rand(s, 7 + i).to(dev) for i, (q, s) in enumerate(dict(pooled=(n, 9, ch), w3=(ch, 9), gamma=(ch,), w1=(ch // 2, ch),
                                                                        w2=(ch, ch // 2), dgate=(n, ch)).items())}
        k = dict(save=_alloc((6 * n * ch + 2 * ch,), dev), dpool=_alloc((n, SLOTS, ch), dev))
        for q, s in dict(dw3=(ch, 9), dgamma=(ch,), dbeta=(ch,), dw1=(ch // 2, ch), db1=(ch // 2,), dw2=(ch, ch // 2), db2=(ch,)).items():
            k[q] = _alloc(s, dev)
        a = dict(pooled=p(d["pooled"]), w3=p(d["w3"]), gamma=p(d["gamma"]), w1=p(d["w1"]), w2=p(d["w2"]), dropmask=NULL, save=p(k["save"][1]),
                 dgate=p(d["dgate"]), dpool=p(k["dpool"][1]), cstride=ch, coff=0, H=6, W=6)
        a.update({q: p(k[q][1]) for q in ("dw3", "dgamma", "dbeta", "dw1", "db1", "dw2", "db2")})
        a.update(N=n, C=ch, stage=0, gsum=NULL, count_scale=C.c_double(1.0), pgrad_scale=C.c_float(1.0), tsum=NULL, pstat=NULL, slices=NULL,
                 stream=_lib.stream())
        fn = L.lhn_ca_mlp_bwd2
    assert set(over) <= set(a), f"{name}: no such argument"
    a.update(over)
    before = [(q, v.clone()) for q, v in _writable(k)]
    torch.cuda.synchronize()
    rc = fn(*a.values())
    err = L.lhn_last_error().decode()
    torch.cuda.synchronize()
    untouched = all(torch.equal(v, w) for (_, v), (_, w) in zip(before, _writable(k)))
    return rc, untouched, err


# ---------------------------------------------------------------- input conditions (CPU)
def _check_reference():
    import time
    t0 = time.time()
    for name, c in CASES.items():
        g = inputs(name)                     # (raises for a case without a valid seed)
        bad = conditions(name, g)
        assert not bad, f"{name}: {bad}"
        r64, r32 = reference(name, g), reference(name, g, torch.float32)
        worst, line = 0.0, []
        for k in r64:
            assert np.isfinite(r64[k]).all(), f"{name} {k}: reference not finite"
            assert np.abs(r64[k]).max() > 0, f"{name} {k}: reference identically zero"
            e = rel_err(r32[k], r64[k])
            worst = max(worst, e)
            if k.split("_")[-1] in ("gate", "dpool"):
                assert e <= FLOOR, f"{name} {k}: the float32 reference misses the floor itself: {e:.2e}"
                line.append(f"{k} {e:.1e}")
        if c.get("zero"):
            for r in (r64, r32):
                for what, v in dead_parts(name, r).items():
                    assert not np.any(v), f"{name}: torch's own {what} is not exactly zero"
        n_dec = sum(int(d.numel()) for _, d in decisions(name, g))
        print(f"{name:24s} seed {g['seed']:4d}, {n_dec:6d} branch decisions, {len(r64):2d} outputs, worst float32 error {worst:.2e}  ({', '.join(line)})")
    print(f"{len(CASES)} cases, input conditions hold, {time.time() - t0:.1f} s")


if __name__ == "__main__":
    if sys.argv[1] == "--check-reference":
        _check_reference()
        sys.exit(0)
    dst, reps, names = sys.argv[1], int(sys.argv[2]), sys.argv[3:]
    dev = torch.device("cuda:0")
    res = {}
    for nm in names:
        base, wrap = nm.split("@")[0], nm.endswith("@wrapper")
        g = inputs(base)
        for r in range(reps):
            for k, v in run(base, dev, g, wrapper=wrap).items():
                res[f"{nm}/{r}/{k}"] = v
    np.savez(dst, **res)
