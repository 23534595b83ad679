"""Cases of the channel-attention MLP (lhn_ca_mlp_fwd / lhn_ca_mlp_bwd2: k_ca1s + k_ca2s and k_ca_bwd2s + k_ca_bwd1s, or the four
kernels they replace under LHN_CA_MLP_V1=1 and for C > 128) run through the C ABI, with a plain torch reference on the CPU: float64,
or float32 to measure what the same operation loses in the kernels' own precision.  The backward reference is torch's autograd of
the forward reference, not a restatement of the kernels' formulas.  Imported by tests/test_ca_mlp_gpu.py; run as a script (a child
process with its own environment, e.g. LHN_CA_MLP_V1=1 or LHN_DETERMINISTIC=1) it writes every output of the named cases to an .npz:
    python tests/ca_mlp_cases.py OUT.npz REPEATS NAME ...
    python tests/ca_mlp_cases.py --check-reference        (CPU only: every case's inputs and both references)
    python tests/ca_mlp_cases.py --train-step OUT.npz     (one small training step end to end, see _train_step)

Inputs.  The hidden layer's bias is +-4 (alternating) under pre-activations of unit scale, so that both leaky-ReLU branches are
taken and no pre-activation sits near the kink: a reference whose float32 form flips a branch would widen the bar and hide a failure.
Pooled values have scale 0.25 (they are bin means of activations)."""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from litehandnet_amd import _lib  # noqa: E402

FLOOR = 2e-5                     # the project's kernel-level floor (test_pw_gpu.FLOOR)
PREFILL = 7.0
PAD = 64                         # floats (doubles) behind every output buffer: must keep their prefill
REPLICAS = 32                    # LHN_STAT_REPLICAS
MARGIN = 1e-3                    # no hidden pre-activation within this of zero (float64)
EPS, MOMENTUM = 1e-5, 0.1
SLOTS = 25                       # LHN_DPOOL_SLOTS


class BnSlices(C.Structure):     # lhn_bn_slices (include/lhn.h)
    _fields_ = [("save", C.c_void_p * 2), ("sums", C.c_void_p * 2), ("lo", C.c_int32 * 2), ("C", C.c_int32 * 2), ("n", C.c_int32)]


# mode: train | eval | deployed (gamma == NULL, bias through beta);  hw: the gated map (bin sizes of the pooled gradient);
# mask: dropout mask;  stat: tsum / pstat with these BatchNorm slices (lo, C);  pre: parameter gradients start non-zero;
# coff / cs: the attention gates channels [coff, coff + c) of a buffer cs wide;  staged: stage 1 then stage 2 (count_scale 1)
CASES = {
    # (N = 2: BatchNorm maps any two samples to +-1, so its input gradient is ~ eps / (var + eps) of its terms -- pure rounding in
    # float32 unless var is of the order of eps: pooled values of scale 0.01 here)
    "n2_c2": dict(n=2, c=2, hw=(6, 6), pscale=0.01),                                 # Ch = 1, one lane of one channel block
    "n5_c34": dict(n=5, c=34, hw=(6, 6)),                                            # partial channel block, more sample lanes than samples
    "n33_c64": dict(n=33, c=64, hw=(6, 6)),                                          # second trip of the sample-lane loop partly filled
    "n70_c16_mask_slices": dict(n=70, c=16, hw=(6, 6), mask=True, stat=[(0, 16)]),   # N > 64: third trip of the sample lanes, second staging round
    "n64_c128_mask_slices": dict(n=64, c=128, hw=(12, 12), mask=True, stat=[(0, 64), (64, 64)], pre=True),   # the benchmark's N x C
    "n3_c256_view": dict(n=3, c=256, hw=(7, 5), coff=8, cs=256 + 16, pre=True),      # uneven, overlapping bins; the largest C
    "n1_c128": dict(n=1, c=128, hw=(6, 6), zero_bwd=True),                           # N = 1 branch of the unbiased variance
    "n1_c128_eval": dict(n=1, c=128, hw=(6, 6), mode="eval"),
    "eval_c64": dict(n=4, c=64, hw=(6, 6), mode="eval"),                             # running statistics
    "deployed_c64": dict(n=4, c=64, hw=(6, 6), mode="deployed"),
    "stage12_c64": dict(n=6, c=64, hw=(6, 6), mask=True, staged=True),               # must give the bits of stage0_c64
    "stage0_c64": dict(n=6, c=64, hw=(6, 6), mask=True, like="stage12_c64"),
}
FWD_KEYS = ("gate", "a", "ahat", "h", "g", "mean", "invstd", "rmean", "rvar")
BWD_KEYS = ("dpool", "dw3", "dgamma", "dbeta", "dw1", "db1", "dw2", "db2", "dahat", "dv", "dh")


def mode(name):
    return CASES[name].get("mode", "train")


def has_bwd(name):
    return mode(name) == "train"


def rel_err(a, b):
    """Max absolute difference over every element, relative to the reference's largest magnitude."""
    return float(np.abs(np.asarray(a, np.float64) - b).max()) / max(float(np.abs(b).max()), 1e-30)


def _rand(shape, seed, scale=1.0):
    return torch.from_numpy((np.random.Generator(np.random.PCG64(seed)).standard_normal(shape) * scale).astype(np.float32))


def _gen(name, seed):
    c = CASES[name]
    n, ch = c["n"], c["c"]
    h = ch // 2
    g = {"seed": seed}
    g["pooled"] = _rand((n, 9, ch), seed, c.get("pscale", 0.25))
    g["w3"] = _rand((ch, 9), seed + 1, 1.0 / 3.0)
    g["gamma"] = 1 + 0.3 * _rand((ch,), seed + 2)
    g["beta"] = 0.5 * _rand((ch,), seed + 3)
    g["rmean"] = 0.1 * _rand((ch,), seed + 4)
    g["rvar"] = 0.05 + 0.02 * _rand((ch,), seed + 5).abs()
    g["w1"] = _rand((h, ch), seed + 6, ch ** -0.5)
    g["b1"] = 4.0 * torch.tensor([1.0 if j % 2 == 0 else -1.0 for j in range(h)]) + 0.2 * _rand((h,), seed + 7)
    g["w2"] = _rand((ch, h), seed + 8, 0.5 * h ** -0.5)
    g["b2"] = 0.3 * _rand((ch,), seed + 9)
    if c.get("mask"):          # Dropout2d(p = 0.3) on the [N, C, 1, 1] tensor: 0 or 1 / 0.7 per (sample, channel)
        keep = torch.from_numpy(np.random.Generator(np.random.PCG64(seed + 10)).random((n, ch)) >= 0.3)
        g["mask"] = keep.float() / 0.7
    g["dgate"] = _rand((n, ch), seed + 11)
    if c.get("stat"):
        g["tsum"] = _rand((n, 2, ch), seed + 12)
        g["pstat"] = _rand((n * 9, 2, ch), seed + 13, 2.0)
    for i, (k, shp) in enumerate((("dw3", (ch, 9)), ("dgamma", (ch,)), ("dbeta", (ch,)), ("dw1", (h, ch)), ("db1", (h,)), ("dw2", (ch, h)), ("db2", (ch,)))):
        g[k + "_0"] = 0.05 * _rand(shp, seed + 20 + i) if c.get("pre") else torch.zeros(shp)
    return g


def hidden_pre(name, g, dtype=torch.float64):
    return _forward(name, {k: (v.to(dtype) if torch.is_tensor(v) else v) for k, v in g.items()})["pre"]


def inputs(name, seed=7):
    """Seeded inputs; a seed at which a hidden pre-activation lies within MARGIN of zero is passed over."""
    name = CASES[name].get("like", name)
    for s in range(seed, seed + 1000, 100):
        g = _gen(name, s)
        if float(hidden_pre(name, g).abs().min()) >= MARGIN:
            return g
    raise AssertionError(f"{name}: no seed keeps the hidden pre-activations away from zero")


# ---------------------------------------------------------------- reference
def _forward(name, t):
    """The attention on the pooled tensor, in the dtype of `t`'s tensors (differentiable)."""
    c = CASES[name]
    n, md = c["n"], mode(name)
    a = (t["pooled"] * t["w3"].t()[None]).sum(1)                       # depthwise 3x3, 'valid', on the 3 x 3 pooled map
    out = {"a": a}
    if md == "deployed":
        mean, var, inv = torch.zeros_like(a[0]), None, torch.ones_like(a[0])
        ahat = a + t["beta"]
    else:
        if md == "train":
            mean = a.mean(0)
            var = ((a - mean) ** 2).mean(0)
            out["rmean"] = (1 - MOMENTUM) * t["rmean"] + MOMENTUM * mean.detach()
            out["rvar"] = (1 - MOMENTUM) * t["rvar"] + MOMENTUM * (var.detach() * n / (n - 1) if n > 1 else var.detach())
        else:
            mean, var = t["rmean"], t["rvar"]
            out["rmean"], out["rvar"] = t["rmean"], t["rvar"]
        inv = 1.0 / torch.sqrt(var + EPS)
        ahat = (a - mean) * inv * t["gamma"] + t["beta"]
    if "mask" in t:
        ahat = ahat * t["mask"]
    pre = ahat @ t["w1"].t() + t["b1"]
    h = torch.where(pre > 0, pre, 0.01 * pre)
    g = torch.sigmoid(h @ t["w2"].t() + t["b2"])
    out.update(ahat=ahat, pre=pre, h=h, g=g, gate=g, mean=mean, invstd=inv)
    return out


def _bins(s):
    return [((i * s) // 3, ((i + 1) * s + 2) // 3) for i in range(3)]


def _dpool25(d9):
    """[N, 9, C] (already divided by the bin sizes) -> the 25 segment sums [N, 25, C] (lhn_dpool_store)."""
    out = torch.zeros(d9.shape[0], SLOTS, d9.shape[2], dtype=d9.dtype)
    for sh in range(5):
        for sw in range(5):
            for bi in range(3):
                for bj in range(3):
                    if sh in (2 * bi - 1, 2 * bi, 2 * bi + 1) and sw in (2 * bj - 1, 2 * bj, 2 * bj + 1):
                        out[:, sh * 5 + sw] += d9[:, bi * 3 + bj]
    return out


def reference(name, g=None, dtype=torch.float64):
    """Every output as numpy float64 arrays, computed in `dtype`."""
    c = CASES[name]
    g = g or inputs(name)
    t = {k: (v.to(dtype) if torch.is_tensor(v) else v) for k, v in g.items()}
    leaves = ("pooled", "w3", "gamma", "beta", "w1", "b1", "w2", "b2")
    if has_bwd(name):
        for k in leaves:
            t[k] = t[k].clone().requires_grad_()
    f = _forward(name, t)
    out = {k: f[k] for k in FWD_KEYS if k in f}
    if mode(name) == "deployed":
        for k in ("rmean", "rvar", "mean", "invstd"):       # (mean = 0 and invstd = 1 are constants there: run() checks them exactly)
            out.pop(k, None)
    if has_bwd(name):
        f["ahat"].retain_grad(), f["h"].retain_grad()
        z = f["h"] @ t["w2"].t() + t["b2"]
        pre = f["pre"]
        pre.retain_grad(), z.retain_grad()
        torch.sigmoid(z).mul(t["dgate"]).sum().backward()
        (hh, ww) = c["hw"]
        binv = torch.tensor([1.0 / ((bh[1] - bh[0]) * (bw[1] - bw[0])) for bh in _bins(hh) for bw in _bins(ww)], dtype=dtype)
        dseg = t["pooled"].grad * binv[None, :, None]
        out["dpool"] = _dpool25(dseg)
        for k in ("w3", "gamma", "beta", "w1", "b1", "w2", "b2"):
            out["d" + k] = t["d" + k + "_0"] + t[k].grad
        # (the scratch rows behind `save`: gradient at ahat before the mask, at the sigmoid's and the leaky ReLU's inputs)
        out["dahat"] = pre.grad @ t["w1"].detach()
        out["dv"], out["dh"] = z.grad, pre.grad
        if c.get("stat"):
            gg, ts, ps = f["g"].detach(), t["tsum"], t["pstat"].view(c["n"], 9, 2, c["c"])
            for k, (lo, cc) in enumerate(c["stat"]):
                for j, nm in enumerate(("du", "duxhat")):
                    tot = (gg * ts[:, j] + (dseg * ps[:, :, j]).sum(1)).sum(0)
                    out[f"sums{k}_{nm}"] = tot[lo:lo + cc]
    return {k: v.detach().double().numpy() for k, v in out.items()}


# ---------------------------------------------------------------- kernels
def _alloc(shape, dev, init=None, dtype=torch.float32, fill=PREFILL):
    """A tensor of `shape` in front of PAD more elements, all `fill` (or `init`): (flat buffer, view)."""
    cnt = int(np.prod(shape))
    flat = torch.full((cnt + PAD,), fill, device=dev, dtype=dtype)
    if init is not None:
        flat[:cnt] = init.reshape(-1).to(dev)
    return flat, flat[:cnt].view(shape)


def _outside(t, coff, c):
    return torch.cat([t[..., :coff], t[..., coff + c:]], -1)


def run(name, dev, g=None):
    """Forward, then (training cases) backward; outputs as numpy arrays plus `*_ok` flags: every float outside an output keeps its
    bits.  `save_all` is the whole save buffer (6 N C + 2 C floats: forward rows and backward scratch)."""
    c = CASES[name]
    g = g or inputs(name)
    d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in g.items()}
    L, st = _lib.lib(), _lib.stream()
    p, fl, dbl = _lib.ptr, C.c_float, C.c_double
    n, ch, md = c["n"], c["c"], mode(name)
    h = ch // 2
    cs, coff = c.get("cs", ch), c.get("coff", 0)
    out = {}
    save_flat, save = _alloc((6 * n * ch + 2 * ch,), dev)
    gate_flat, gate = _alloc((n, cs), dev)
    rm_flat, rmean = _alloc((ch,), dev, d["rmean"])
    rv_flat, rvar = _alloc((ch,), dev, d["rvar"])
    nbt = torch.full((1 + PAD,), 5, dtype=torch.int64, device=dev)
    gsum = torch.full((2 * ch + PAD,), PREFILL, dtype=torch.float64, device=dev)
    mask = d.get("mask")
    gamma = None if md == "deployed" else d["gamma"]
    train = 1 if md == "train" else 0

    def fwd(stage):
        _lib.check(L.lhn_ca_mlp_fwd(p(d["pooled"]), p(d["w3"]), p(gamma), p(d["beta"]), p(None if gamma is None else rmean),
                                    p(None if gamma is None else rvar), p(nbt if train else None), p(d["w1"]), p(d["b1"]), p(d["w2"]),
                                    p(d["b2"]), p(mask), p(gate), cs, coff, p(save), n, ch, fl(EPS), fl(MOMENTUM), train, stage,
                                    p(gsum if stage else None), dbl(1.0), st), f"lhn_ca_mlp_fwd {name}")
    if c.get("staged"):
        fwd(1)
        fwd(2)
    else:
        fwd(0)
    torch.cuda.synchronize()
    nc, nh = n * ch, n * h
    parts = {"a": (0, (n, ch)), "ahat": (nc, (n, ch)), "h": (2 * nc, (n, h)), "g": (2 * nc + nh, (n, ch)), "mean": (3 * nc + nh, (ch,)),
             "invstd": (3 * nc + nh + ch, (ch,))}
    for k, (o, shp) in parts.items():
        out[k] = save[o:o + int(np.prod(shp))].view(shp).cpu().numpy()
    out["gate"] = gate[:, coff:coff + ch].cpu().numpy()
    out["gate_ok"] = np.array(bool((gate_flat[n * cs:] == PREFILL).all()) and bool((_outside(gate, coff, ch) == PREFILL).all()))
    if md != "deployed":
        out["rmean"], out["rvar"] = rmean.cpu().numpy(), rvar.cpu().numpy()
    out["stats_ok"] = np.array(bool((rm_flat[ch:] == PREFILL).all()) and bool((rv_flat[ch:] == PREFILL).all()) and bool((nbt[1:] == 5).all())
                               and (md != "deployed" or (torch.equal(rmean, d["rmean"]) and torch.equal(rvar, d["rvar"]))))
    out["nbt"] = nbt[:1].cpu().numpy()
    if md == "deployed":
        out["const_ok"] = np.array(bool((save[3 * nc + nh:3 * nc + nh + ch] == 0).all()) and bool((save[3 * nc + nh + ch:3 * nc + nh + 2 * ch] == 1).all()))
    fwd_scratch_ok = bool((save[3 * nc + nh + 2 * ch:] == PREFILL).all())            # the forward leaves the backward's scratch alone
    if has_bwd(name):
        grads = {}
        for k in ("dw3", "dgamma", "dbeta", "dw1", "db1", "dw2", "db2"):
            grads[k] = _alloc(tuple(g[k + "_0"].shape), dev, g[k + "_0"])
        dp_flat, dpool = _alloc((n, SLOTS, cs), dev)
        sl, sums = None, []
        if c.get("stat"):
            sl = BnSlices()
            sl.n = len(c["stat"])
            dummy = torch.zeros(2 * ch, device=dev)
            for k, (lo, cc) in enumerate(c["stat"]):
                sums.append(torch.zeros(REPLICAS * 2 * cc + PAD, dtype=torch.float64, device=dev))
                sl.save[k], sl.sums[k], sl.lo[k], sl.C[k] = dummy.data_ptr(), sums[k].data_ptr(), lo, cc

        def bwd(stage):
            _lib.check(L.lhn_ca_mlp_bwd2(p(d["pooled"]), p(d["w3"]), p(d["gamma"]), p(d["w1"]), p(d["w2"]), p(mask), p(save), p(d["dgate"]),
                                         p(dpool), cs, coff, c["hw"][0], c["hw"][1], *[p(grads[k][1]) for k in ("dw3", "dgamma", "dbeta", "dw1", "db1", "dw2", "db2")],
                                         n, ch, stage, p(gsum if stage else None), dbl(1.0), fl(1.0), p(d.get("tsum")), p(d.get("pstat")),
                                         C.byref(sl) if sl is not None else None, st), f"lhn_ca_mlp_bwd2 {name}")
        if c.get("staged"):
            bwd(1)
            bwd(2)
        else:
            bwd(0)
        torch.cuda.synchronize()
        ok = True
        for k, (flat, t) in grads.items():
            out[k] = t.cpu().numpy()
            ok = ok and bool((flat[t.numel():] == PREFILL).all())
        out["grads_ok"] = np.array(ok)
        out["dpool"] = dpool[:, :, coff:coff + ch].cpu().numpy()
        out["dpool_ok"] = np.array(bool((dp_flat[dpool.numel():] == PREFILL).all()) and bool((_outside(dpool, coff, ch) == PREFILL).all()))
        o = 3 * nc + nh + 2 * ch
        out["dahat"] = save[o:o + nc].view(n, ch).cpu().numpy()
        out["dv"] = save[o + nc:o + 2 * nc].view(n, ch).cpu().numpy()
        out["dh"] = save[o + 2 * nc:o + 2 * nc + nh].view(n, h).cpu().numpy()
        for k, (lo, cc) in enumerate(c.get("stat", [])):
            t = sums[k][:REPLICAS * 2 * cc].view(REPLICAS, 2, cc)
            out[f"sums{k}_du"], out[f"sums{k}_duxhat"] = t[0, 0].cpu().numpy(), t[0, 1].cpu().numpy()
            out[f"sums{k}_ok"] = np.array(bool((t[1:] == 0).all()) and bool((sums[k][t.numel():] == 0).all()))     # replica 0 only
    out["save_all"] = save.cpu().numpy()
    out["save_ok"] = np.array(bool((save_flat[save.numel():] == PREFILL).all()) and fwd_scratch_ok)
    out["gsum_ok"] = np.array(bool((gsum[2 * ch:] == PREFILL).all()) and (bool(c.get("staged")) or bool((gsum == PREFILL).all())))
    return out


# ---------------------------------------------------------------- input conditions (CPU)
def _check_reference():
    import time
    t0 = time.time()
    for name, c in CASES.items():
        g = inputs(name)
        pre64, pre32 = hidden_pre(name, g), hidden_pre(name, g, torch.float32)
        assert float(pre64.abs().min()) >= MARGIN, f"{name}: a hidden pre-activation within {MARGIN} of zero"
        assert torch.equal(pre64 > 0, pre32 > 0), f"{name}: float32 and float64 disagree about a leaky-ReLU branch"
        assert c["c"] == 2 or (bool((pre64 > 0).any()) and bool((pre64 < 0).any())), f"{name}: one leaky-ReLU branch is never taken"
        r64, r32 = reference(name, g), reference(name, g, torch.float32)
        worst, line = 0.0, []
        for k in r64:
            assert np.isfinite(r64[k]).all(), f"{name} {k}: reference not finite"
            zero = not np.abs(r64[k]).max() > 0
            allowed = bool(c.get("zero_bwd")) and k in ("dpool", "dw3", "dgamma")          # N = 1: the BatchNorm backward returns exact zeros
            assert zero == allowed, f"{name} {k}: reference identically zero: {zero}"
            e = rel_err(r32[k], r64[k])
            worst = max(worst, e)
            if k in ("gate", "dpool"):
                assert allowed or e <= FLOOR, f"{name} {k}: the float32 reference misses the floor itself: {e:.2e}"
                line.append(f"{k} {e:.1e}")
        print(f"{name:22s} {len(r64):2d} outputs, worst float32 error {worst:.2e}  ({', '.join(line)})")
    print(f"{len(CASES)} cases, input conditions hold, {time.time() - t0:.1f} s")


def _train_step(dst):
    """One training step of a model of one MSRB and one gated RepBasicUnit (64 channels, batch 4, 16 x 16 map, dropout live under a
    fixed seed) on seeded inputs: loss, every gradient (and all of them as one flat vector), the input gradient and every buffer."""
    from litehandnet_amd.engine import PlanModule
    from litehandnet_amd.litehourglass import MSRB, RepBasicUnit
    from oracle import synth

    class Tiny(PlanModule):
        def __init__(self):
            super().__init__()
            self.msrb = MSRB(64, 64, "ca", p_drop=0.3)
            self.unit = RepBasicUnit(64, 64, "ca", p_drop=0.3)

        def emit(self, pb, x, out=None):
            return self.unit.emit(pb, self.msrb.emit(pb, x), out=out)

    dev = torch.device("cuda:0")
    m = Tiny()
    m.load_state_dict({k: v.clone() for k, v in synth.synth_state_dict(m, 5).items()})
    m.to(dev).train()
    torch.manual_seed(11)
    x = torch.randn(4, 64, 16, 16, generator=torch.Generator().manual_seed(7)).to(dev).requires_grad_()
    t = torch.randn(4, 64, 16, 16, generator=torch.Generator().manual_seed(3)).to(dev)
    y = m(x)
    loss = ((y - t) ** 2).mean()
    m.zero_grad()
    loss.backward()
    out = {"loss": np.float64(float(loss)), "y": y.detach().cpu().numpy(), "dx": x.grad.detach().cpu().numpy()}
    flat = []
    for k, p in m.named_parameters():
        out[f"g.{k}"] = p.grad.detach().cpu().numpy()
        flat.append(out[f"g.{k}"].reshape(-1))
    out["gflat"] = np.concatenate(flat)
    for k, b in m.named_buffers():
        out[f"b.{k}"] = b.detach().cpu().numpy()
    np.savez(dst, **out)


if __name__ == "__main__":
    if sys.argv[1] == "--check-reference":
        _check_reference()
        sys.exit(0)
    if sys.argv[1] == "--train-step":
        _train_step(sys.argv[2])
        sys.exit(0)
    dst, reps, names = sys.argv[1], int(sys.argv[2]), sys.argv[3:]
    dev = torch.device("cuda:0")
    res = {}
    for nm in names:
        g = inputs(nm)
        for r in range(reps):
            for k, v in run(nm, dev, g).items():
                res[f"{nm}/{r}/{k}"] = v
    np.savez(dst, **res)
