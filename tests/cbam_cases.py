"""Cases, inputs, float64 reference and C-ABI runner of the CBAM kernels (csrc/k_cbam.hip: lhn_cbam_fwd / lhn_cbam_bwd), shared by
tests/test_cbam_gpu.py and its LHN_DETERMINISTIC=1 child process.

    python tests/cbam_cases.py --check-reference      CPU: the inputs of every case are free of chaotic points; prints the worst
                                                      float32-on-the-CPU error of the reference (the yardstick of the bar)
    python tests/cbam_cases.py OUT.npz NAME...        GPU: run the named cases, save every output (the child process)

Arithmetic (attention.py:234-294), p = the VALUE of pre's output, r = residual_conv(x), J = C / 16:
    g = sigmoid(W2 relu(W1 mean_hw p) + W2 relu(W1 max_hw p));  u = g p;  s = [mean_c u, max_c u];
    a = sigmoid(conv7x7(s, zero padding 3));  out = relu(a u + r)
The backward is torch autograd over the same float64 graph (max routes its gradient to the arg-max element).

Chaotic points are removed from the INPUTS: the seed of each case is one for which no runner-up of either maximum lies within
TIE of the winner, no hidden pre-activation of the MLP within TIE of zero (relative to the tensor's largest magnitude) and, so
that dW1 and dW2 are not identically zero, every sample has a live hidden neuron on both paths of the MLP (J is 1 or 2 in the
small cases).  dout is zeroed where |z| < TIE * max|z| in float64 (a ReLU derivative that could flip then multiplies zero; at most 0.1 % of it)."""
import ctypes as C
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

TIE = 2e-5
PREFILL = 7.0
# (N, C, H, W): J = 1 and a single pixel | every 7x7 window clipped on all sides | one row and one column past an 8 x 32 tile |
# fewer rows than the halo | the model's width | the same, 4 x 1 tiles.  Then the paths those six do not take: more than 1024
# pixels (the pooling pass splits each sample over two workgroups), C / 4 = 12 (no power of two: idle lanes in every layout) and
# C = 256 (one pixel per wave)
SHAPES = {"n2c16_1x1": (2, 16, 1, 1), "n2c32_7x7": (2, 32, 7, 7), "n3c32_9x33": (3, 32, 9, 33), "n2c64_5x40": (2, 64, 5, 40),
          "n2c128_14x14": (2, 128, 14, 14), "n1c128_28x28": (1, 128, 28, 28),
          "n1c16_33x40": (1, 16, 33, 40), "n2c48_3x5": (2, 48, 3, 5), "n1c256_2x3": (1, 256, 2, 3)}
# per case: the smallest seed for which `--check-reference` holds (the conditions of the module docstring)
SEEDS = {"n2c16_1x1": 11, "n2c32_7x7": 0, "n3c32_9x33": 1, "n2c64_5x40": 0, "n2c128_14x14": 0, "n1c128_28x28": 1,
         "n1c16_33x40": 2, "n2c48_3x5": 4, "n1c256_2x3": 0, "n3c32_9x33+negtable": 2}
NEG_TABLE = "n3c32_9x33+negtable"       # the same shape behind a table whose scales are negative on every other channel
NAMES = list(SHAPES) + [NEG_TABLE]
OUTPUTS = ("g", "s", "a", "out", "dp", "dr", "dw1", "dw2", "dw7")
INDEXES = ("amax", "cidx")


def _shape(name):
    return SHAPES[name.split("+")[0]]


def inputs(name, seed=None):
    """Host tensors of a case (float32): raw p and its table (scale, shift; slope 1), r, dout before zeroing, the weights."""
    N, Cc, H, W = _shape(name)
    J = Cc // 16
    gen = torch.Generator().manual_seed(1000 + (SEEDS[name] if seed is None else seed))
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32)
    val = 1.5 * rn(N, H, W, Cc) + 0.3
    if name.endswith("+negtable"):
        sc = (0.5 + torch.rand(Cc, generator=gen)) * torch.where(torch.arange(Cc) % 2 == 0, -1.0, 1.0)
        sh = 0.5 * rn(Cc)
    else:
        sc, sh = torch.ones(Cc), torch.zeros(Cc)
    g = dict(p_raw=((val - sh) / sc).contiguous(), sc=sc.float(), sh=sh.float(), r=rn(N, H, W, Cc), dout=rn(N, H, W, Cc),
             w1=rn(J, Cc) / Cc ** 0.5, w2=rn(Cc, J), w7=0.2 * rn(1, 2, 7, 7))
    return g


def forward(g, dt):
    """The formulas in dtype dt on the CPU, NHWC.  Returns a dict of every intermediate (torch tensors, graph attached)."""
    p = (g["p_raw"].to(dt) * g["sc"].to(dt) + g["sh"].to(dt)).requires_grad_()
    r = g["r"].to(dt).requires_grad_()
    w1, w2, w7 = (g[k].to(dt).requires_grad_() for k in ("w1", "w2", "w7"))
    N, H, W, Cc = p.shape
    flat = p.reshape(N, H * W, Cc)
    avg = flat.mean(dim=1)
    mx, amax = flat.max(dim=1)
    ha, hm = avg @ w1.t(), mx @ w1.t()
    gate = torch.sigmoid(F.relu(ha) @ w2.t() + F.relu(hm) @ w2.t())
    u = gate[:, None, None, :] * p
    s1, cidx = u.max(dim=3)
    s = torch.stack([u.mean(dim=3), s1], dim=3)
    a = torch.sigmoid(F.conv2d(s.permute(0, 3, 1, 2), w7, padding=3))[:, 0]
    z = a[..., None] * u + r
    return dict(p=p, r=r, w1=w1, w2=w2, w7=w7, avg=avg, mx=mx, amax=amax, ha=ha, hm=hm, g=gate, u=u, s=s, cidx=cidx, a=a, z=z,
                out=F.relu(z))


def dout_of(g, z64):
    """(dout with the near-zero pre-activations zeroed, how many elements that were)."""
    near = z64.detach().abs() < TIE * z64.detach().abs().max()
    return torch.where(near, torch.zeros(()), g["dout"]), int(near.sum())


def reference(name, g=None, dtype=torch.float64, dout=None):
    """Every output as numpy (float64 or float32 arithmetic); dout defaults to the float64 run's zeroing."""
    g = inputs(name) if g is None else g
    if dout is None:
        dout, _ = dout_of(g, forward(g, torch.float64)["z"])
    f = forward(g, dtype)
    f["out"].backward(dout.to(dtype))
    res = {k: f[k].detach().numpy() for k in ("g", "s", "a", "out")}
    res.update(dp=f["p"].grad.numpy(), dr=f["r"].grad.numpy(), dw1=f["w1"].grad.numpy(), dw2=f["w2"].grad.numpy(),
               dw7=f["w7"].grad.numpy(), amax=f["amax"].numpy().astype(np.int64), cidx=f["cidx"].numpy().astype(np.int64))
    return res


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def chaos(name, g=None):
    """(smallest relative gap of either maximum to its runner-up, smallest relative |hidden pre-activation|, zeroed dout fraction,
    every sample has a positive hidden pre-activation on the mean path and on the max path)."""
    g = inputs(name) if g is None else g
    f = forward(g, torch.float64)
    gaps = []
    for t, dim in ((f["p"].detach().reshape(f["p"].shape[0], -1, f["p"].shape[3]), 1), (f["u"].detach(), 3)):
        if t.shape[dim] > 1:
            top = t.topk(2, dim=dim).values
            gaps.append(float((top.select(dim, 0) - top.select(dim, 1)).min() / t.abs().max()))
    h = torch.cat([f["ha"].detach().flatten(), f["hm"].detach().flatten()])
    _, nz = dout_of(g, f["z"])
    live = bool((f["ha"] > 0).any(dim=1).all() and (f["hm"] > 0).any(dim=1).all())
    return min(gaps) if gaps else float("inf"), float(h.abs().min() / h.abs().max()), nz / f["z"].numel(), live


def check_reference():
    worst = 0.0
    for name in NAMES:
        g = inputs(name)
        gap, hid, frac, live = chaos(name, g)
        r64, r32 = reference(name, g), reference(name, g, torch.float32)
        e32 = {k: rel_err(r32[k], r64[k]) for k in OUTPUTS}
        worst = max(worst, max(e32.values()))
        print(f"{name}: max gap {gap:.2e}, hidden {hid:.2e}, dout zeroed {100 * frac:.4f} %, float32 worst {max(e32.values()):.2e} "
              f"({max(e32, key=e32.get)})")
        assert gap >= TIE and hid >= TIE and frac <= 1e-3 and live, (name, gap, hid, frac, live)
        assert all(np.abs(r64[k]).max() > 0 for k in OUTPUTS), name
        assert all(np.array_equal(r32[k], r64[k]) for k in INDEXES), name
    print(f"worst float32-on-the-CPU error over all cases and outputs: {worst:.2e}")
    return worst


# ---------------------------------------------------------------- GPU runner
def _view(_lib, t, coff, c, table=None):
    N, H, W, cs = t.shape
    return _lib.View(t.data_ptr(), table.data_ptr() if table is not None else None, None, N, H, W, cs, coff, c, None)


def _outside_ok(t, coff, c):
    m = torch.ones(t.shape[-1], dtype=torch.bool)
    m[coff:coff + c] = False
    return bool((t.cpu()[..., m] == PREFILL).all())


def run(name, dev, g=None, reps=1, null_scratch=False, shape=None):
    """lhn_cbam_fwd then lhn_cbam_bwd through the C ABI on views into sentinel-filled buffers.  Returns (status of the forward,
    status of the backward, dict of outputs as numpy + `*_ok` flags for the floats around them); reps > 1: the list of such dicts."""
    from litehandnet_amd import _lib
    L = _lib.lib()
    N, Cc, H, W = shape or _shape(name)
    if g is None:
        g = inputs(name)
    PAD = 8
    dout, _ = dout_of(g, forward(g, torch.float64)["z"]) if shape is None else (g["dout"], 0)
    sv, sc = _lib.cbam_layout(N, H, W, Cc if (Cc % 16 == 0 and Cc <= 256) else 256)      # (an unsupported C: room to spare)
    if shape is not None:
        sv, sc = [2 * x for x in sv], [2 * x for x in sc]

    def buf(src, coff):
        t = torch.full((N, H, W, Cc + PAD), PREFILL, dtype=torch.float32)
        if src is not None:
            t[..., coff:coff + Cc] = src
        return t.to(dev)

    outs = []
    for _ in range(reps):
        pb, rb, ob, dob = buf(g["p_raw"], 4), buf(g["r"], 0), buf(None, 8), buf(dout, 8)
        dpb, drb = buf(None, 4), buf(None, 0)
        tab = torch.ones(3, Cc + PAD)
        tab[0, 4:4 + Cc], tab[1, 4:4 + Cc] = g["sc"], g["sh"]
        tab[1, :4], tab[1, 4 + Cc:] = 0.0, 0.0
        tab = tab.to(dev)
        w1, w2, w7 = g["w1"].to(dev), g["w2"].to(dev), g["w7"].to(dev)
        dw1, dw2, dw7 = torch.zeros_like(w1), torch.zeros_like(w2), torch.zeros_like(w7)
        save = torch.full((sv[-1] + 16,), PREFILL, dtype=torch.float32, device=dev)
        scr = torch.full((sc[-1] + 16,), PREFILL, dtype=torch.float32, device=dev)
        pv, rv, ov = _view(_lib, pb, 4, Cc, tab), _view(_lib, rb, 0, Cc), _view(_lib, ob, 8, Cc)
        st = _lib.stream()
        rc_f = L.lhn_cbam_fwd(C.byref(pv), C.byref(rv), _lib.ptr(w1), _lib.ptr(w2), _lib.ptr(w7), C.byref(ov), _lib.ptr(save), st)
        rc_b = L.lhn_cbam_bwd(C.byref(pv), C.byref(rv), _lib.ptr(w1), _lib.ptr(w2), _lib.ptr(w7), C.byref(ov), _lib.ptr(dob),
                              _lib.ptr(dpb), _lib.ptr(drb), _lib.ptr(dw1), _lib.ptr(dw2), _lib.ptr(dw7), _lib.ptr(save),
                              None if null_scratch else _lib.ptr(scr), st)
        torch.cuda.synchronize()
        sh = save.cpu()
        untouched = bool((ob.cpu() == PREFILL).all() and (dpb.cpu() == PREFILL).all() and (drb.cpu() == PREFILL).all()
                         and (sh == PREFILL).all() and (scr.cpu() == PREFILL).all() and not dw1.any() and not dw2.any() and not dw7.any())
        if shape is not None:
            outs.append((rc_f, rc_b, dict(untouched=untouched, error=L.lhn_last_error().decode())))
            continue
        cut = lambda k, n: sh[sv[k]:sv[k] + n]
        res = dict(g=cut(4, N * Cc).view(N, Cc).numpy(), s=cut(5, N * H * W * 2).view(N, H, W, 2).numpy(), a=cut(7, N * H * W).view(N, H, W).numpy(),
                   amax=cut(2, N * Cc).view(torch.int32).view(N, Cc).numpy().astype(np.int64),
                   cidx=cut(6, N * H * W).view(torch.int32).view(N, H, W).numpy().astype(np.int64),
                   out=ob.cpu()[..., 8:8 + Cc].numpy(), dp=dpb.cpu()[..., 4:4 + Cc].numpy(), dr=drb.cpu()[..., 0:Cc].numpy(),
                   dw1=dw1.cpu().numpy(), dw2=dw2.cpu().numpy(), dw7=dw7.cpu().numpy())
        res.update(out_ok=_outside_ok(ob, 8, Cc), dp_ok=_outside_ok(dpb, 4, Cc), dr_ok=_outside_ok(drb, 0, Cc),
                   p_ok=bool((pb.cpu() == buf(g["p_raw"], 4).cpu()).all()), dout_ok=bool((dob.cpu() == buf(dout, 8).cpu()).all()),
                   save_ok=bool((sh[sv[-1]:] == PREFILL).all()), scratch_ok=bool((scr.cpu()[sc[-1]:] == PREFILL).all()),
                   bwd_untouched=bool((dpb.cpu() == PREFILL).all() and (drb.cpu() == PREFILL).all() and (scr.cpu() == PREFILL).all()
                                      and not dw1.any() and not dw2.any() and not dw7.any()))
        outs.append((rc_f, rc_b, res))
    return outs[0] if reps == 1 else outs


def refusal_inputs(shape, seed=0):
    """Random inputs of an unsupported shape (never compared with a reference)."""
    N, Cc, H, W = shape
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32)
    J = max(Cc // 16, 1)
    return dict(p_raw=rn(N, H, W, Cc), sc=torch.ones(Cc), sh=torch.zeros(Cc), r=rn(N, H, W, Cc), dout=rn(N, H, W, Cc),
                w1=rn(J, Cc), w2=rn(Cc, J), w7=rn(1, 2, 7, 7))


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1:] == ["--check-reference"]:
        check_reference()
    else:
        dev = torch.device("cuda:0")
        saved = {}
        for nm in sys.argv[2:]:
            rc_f, rc_b, res = run(nm, dev)
            assert rc_f == 0 and rc_b == 0, (nm, rc_f, rc_b)
            saved.update({f"{nm}/{k}": np.asarray(v) for k, v in res.items()})
        np.savez(sys.argv[1], **saved)
