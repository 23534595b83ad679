"""Cases of what stands between a convolution and its BatchNorm (csrc/k_misc.hip): lhn_bn_bwd_reduce with and without its fused
finalize (lhn_bnbwdfin), lhn_bn_finalize2, lhn_bn_bwd_finalize2, lhn_fold_stat_replicas and lhn_reduce_replicas, run through the C
ABI, with a plain torch / numpy reference on the CPU (float64, or float32 to measure what the same operation loses in the kernels'
own precision).  Imported by tests/test_bn_gpu.py; run as a script (a child process under LHN_DETERMINISTIC=1) it writes the kernel
outputs of the named cases to an .npz file:
    python tests/bn_cases.py OUT.npz REPEATS NAME ...
    python tests/bn_cases.py --check-reference        (CPU only: every case's inputs, both references, the branch each one reaches)

kernel_of(name) repeats the launchers' dispatch and says which reduction of k_bn_bwd_reduce a case takes."""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pw_cases import PREFILL, _dact, _kinks, _lib, _outside, _rand, _seg, _tab, _view, rel_err  # noqa: E402,F401
from dw_fwd_cases import STAT_PAD, STAT_REPLICAS, TICKET_WORDS  # noqa: E402
from litehandnet_amd._lib import GradView  # noqa: E402

EPS, MOMENTUM, SLOPE = 1e-5, 0.1, 0.1
FIN_THREADS = 1024               # LHN_FIN_THREADS (csrc/lhn_common.h)
NPIX = 53                        # pixels behind the synthetic statistics of the finalize cases


class BnBwdFin(C.Structure):     # lhn_bnbwdfin (include/lhn.h)
    _fields_ = [("counter", C.c_void_p), ("gamma", C.c_void_p), ("coef", C.c_void_p), ("dgamma", C.c_void_p), ("dbeta", C.c_void_p),
                ("count", C.c_double), ("cstride", C.c_int32), ("coff", C.c_int32), ("C", C.c_int32)]


def _red(n, h, w, cs, coff, c, flags="", **kw):
    return dict(op="reduce", n=n, h=h, w=w, cs=cs, coff=coff, c=c, flags=flags.split(), **kw)


def _fz(c, sc, flags="", op="finalize", **kw):
    """Finalize cases work on channels [8, 8 + c) of a table of c + 12."""
    return dict(op=op, c=c, sc=sc, cs=c + 12, coff=8, flags=flags.split(), **kw)


CASES = {}
# 1. lhn_bn_bwd_reduce.  flags: gate / dpool on y;  notab: y without a table;  fin: fused finalize (lhn_bnbwdfin)
CASES["r_c32"] = _red(2, 16, 16, 32, 0, 32)                          # shuffle reduction, C4 = 8
CASES["r_c64_view"] = _red(2, 9, 13, 96, 32, 64, "gate dpool")       # C4 = 16, slice view
CASES["r_c128_w37"] = _red(1, 5, 37, 128, 0, 128, "gate")            # PL = 8: W > 4 PL, second pass with clamped tail loads
CASES["r_c16"] = _red(2, 7, 5, 16, 0, 16)                            # C4 = 4
CASES["r_c4"] = _red(3, 3, 3, 8, 4, 4, "notab")                      # C4 = 1
CASES["r_c20"] = _red(2, 5, 7, 40, 8, 20, "gate dpool")              # C4 = 5: LDS fold, thread 255 dead
CASES["r_c40"] = _red(2, 5, 7, 40, 0, 40)                            # C4 = 10: threads 250.. dead
CASES["r_c256"] = _red(1, 4, 4, 256, 0, 256, "dpool")                # C4 = 64
CASES["r_c320"] = _red(1, 3, 5, 320, 0, 320)                         # PL = 3, 16 dead threads
CASES["r_c1024"] = _red(1, 2, 3, 1024, 0, 1024)                      # PL = 1
CASES["r_w3"] = _red(3, 4, 3, 64, 0, 64, "gate")                     # W < PL
CASES["r_rows"] = _red(2, 40, 8, 32, 0, 32)                          # 80 rows: the row loop in deterministic mode
REDUCE_CASES = list(CASES)
for _n in ("r_c32", "r_c20", "r_c256"):                              # the same three with the fused finalize
    CASES[_n.replace("r_", "rf_")] = dict(CASES[_n], flags=CASES[_n]["flags"] + ["fin"])
FUSED_CASES = [n for n in CASES if n.startswith("rf_")]

# 2. lhn_bn_finalize2 (C, stat_channels).  flags: bias: conv_bias;  noaffine: gamma = beta = NULL;  norun: no running statistics;
#    count1: one pixel;  const: channel 3 is constant (var < 0 clamp, invstd = 1 / sqrt(eps));  eval: table from the running statistics
CASES["fz_c7"] = _fz(7, 8, "bias const")
CASES["fz_c32"] = _fz(32, 32, "noaffine")
CASES["fz_c37"] = _fz(37, 40, "norun")
CASES["fz_c40"] = _fz(40, 40, "count1")
CASES["fz_c256"] = _fz(256, 256, "const")
CASES["fz_c1024"] = _fz(1024, 1024, "bias")
CASES["fz_c1028"] = _fz(1028, 1028)                                  # the second round of the c0 loop
CASES["fz_eval_c37"] = _fz(37, 40, "eval bias")
CASES["fz_eval_c256"] = _fz(256, 256, "eval")
# 3. lhn_bn_bwd_finalize2.  flags: nogamma;  pgrad: pgrad_scale = 0.5;  nograd: dgamma = dbeta = NULL (else: added to a prior)
CASES["bz_c7"] = _fz(7, 8, "pgrad", op="bwd_finalize")
CASES["bz_c32"] = _fz(32, 32, "nogamma", op="bwd_finalize")
CASES["bz_c37"] = _fz(37, 40, "nograd", op="bwd_finalize")
CASES["bz_c40"] = _fz(40, 40, op="bwd_finalize")
CASES["bz_c256"] = _fz(256, 256, "pgrad nogamma", op="bwd_finalize")
CASES["bz_c1024"] = _fz(1024, 1024, op="bwd_finalize")
CASES["bz_c1028"] = _fz(1028, 1028, "pgrad", op="bwd_finalize")
# 4. lhn_fold_stat_replicas: n doubles x 32 replicas (16400 > 64 workgroups x 256: the grid-stride loop)
for _n in (14, 64, 16400):
    CASES[f"fold_{_n}"] = dict(op="fold", n=_n, nrep=STAT_REPLICAS, flags=[])
# 5. lhn_reduce_replicas: rep_stride = n + 8;  alias: out is replica 0
for _n, _r, _a in ((4, 1, ""), (4, 4, "alias"), (4, 16, ""), (1000, 1, "alias"), (1000, 4, ""), (1000, 16, "alias")):
    CASES[f"repl_{_n}_{_r}"] = dict(op="repl", n=_n, nrep=_r, flags=_a.split())

# calls the library must refuse (non-zero status, the reason in lhn_last_error, nothing written)
REFUSE = {
    "fin_C": dict(_red(2, 5, 7, 40, 8, 20, "fin"), fin_slice=(40, 8, 16), refuse="fused finalize slice"),
    "fin_coff": dict(_red(2, 5, 7, 40, 8, 20, "fin"), fin_slice=(40, 4, 20), refuse="fused finalize slice"),
    "fin_cstride": dict(_red(2, 5, 7, 40, 8, 20, "fin"), fin_slice=(48, 8, 20), refuse="fused finalize slice"),
    "repl_n6": dict(op="repl", n=6, nrep=4, flags=[], refuse="multiples of 4"),
}
_ALL = dict(CASES, **REFUSE)


def kernel_of(name, gather=False):
    """The kernel a case launches and the branch it takes (none of them looks at LHN_DW_GATHER)."""
    c = _ALL[name]
    if c["op"] == "reduce":
        c4 = c["c"] // 4
        how = "shuffle" if c4 <= 32 and c4 & (c4 - 1) == 0 else f"LDS fold, {256 - 256 // c4 * c4} dead threads"
        return f"k_bn_bwd_reduce C4={c4} PL={256 // c4} {how}" + (" + lhn_bn_bwd_finalize_block" if "fin" in c["flags"] else "")
    if c["op"] == "finalize":
        return f"k_bn_finalize {'eval' if 'eval' in c['flags'] else 'G=%d' % max(1, min(STAT_REPLICAS, FIN_THREADS // c['c']))}"
    if c["op"] == "bwd_finalize":
        return f"k_bn_bwd_finalize G={max(1, min(STAT_REPLICAS, FIN_THREADS // c['c']))} rounds={(c['c'] + FIN_THREADS - 1) // FIN_THREADS}"
    return {"fold": "k_fold_stat_replicas", "repl": "k_reduce_replicas"}[c["op"]]


def _split(tot, seed):
    """[32][...] doubles that add up to `tot` (float64) up to rounding: random shares per replica."""
    r = np.random.Generator(np.random.PCG64(seed)).random((STAT_REPLICAS,) + tot.shape) + 0.1
    return torch.from_numpy(r / r.sum(0) * tot.numpy())


def _gen(name, seed):
    c = _ALL[name]
    f, op = c["flags"], c["op"]
    g = {"seed": seed}
    if op == "reduce":
        n, h, w, cs, ch = c["n"], c["h"], c["w"], c["cs"], c["c"]
        g["y"], g["dz"] = _rand((n, h, w, cs), seed), _rand((n, h, w, cs), seed + 2)
        if "notab" not in f:
            g["ytab"] = _tab(cs, seed + 6)
        if "gate" in f:
            g["ygate"] = torch.sigmoid(_rand((n, cs), seed + 12))
        if "dpool" in f:
            g["dpool"] = 0.3 * _rand((n, 25, cs), seed + 13)
        g["save"] = torch.stack([0.1 * _rand((ch,), seed + 20), 1 + 0.2 * _rand((ch,), seed + 21).abs()]).contiguous()
        if "fin" in f:
            g["gamma"] = 1 + 0.2 * _rand((ch,), seed + 60)
            g["dgamma0"], g["dbeta0"] = _rand((ch,), seed + 65), _rand((ch,), seed + 66)
    elif op == "finalize":
        ch, sc = c["c"], c["sc"]
        npix = 1 if "count1" in f else NPIX
        x = 0.3 * _rand((sc,), seed + 1) + (1 + 0.2 * _rand((sc,), seed + 2).abs()) * _rand((npix, sc), seed)
        if "const" in f:
            x[:, 3] = 1.7
        g["x"] = x                                                        # the data the statistics are of
        x64 = x.double()
        tot = torch.stack([x64.sum(0), (x64 * x64).sum(0)])               # [2][SC]
        g["stats"] = _split(tot, seed + 5) if npix > 1 else torch.cat([tot[None], torch.zeros(STAT_REPLICAS - 1, 2, sc, dtype=torch.float64)])
        if "const" in f:                                                  # exactly n v | n v^2, all of it in replica 0
            g["stats"][:, :, 3] = 0
            g["stats"][0, 0, 3], g["stats"][0, 1, 3] = npix * float(x[0, 3]), npix * float(x[0, 3]) ** 2
        if "noaffine" not in f:
            g["gamma"], g["beta"] = 1 + 0.2 * _rand((ch,), seed + 60), 0.3 * _rand((ch,), seed + 61)
        g["rmean"], g["rvar"] = 0.1 * _rand((ch,), seed + 62), 1 + 0.2 * _rand((ch,), seed + 63).abs()
        if "bias" in f:
            g["cbias"] = 0.5 * _rand((ch,), seed + 64)
    elif op == "bwd_finalize":
        ch, sc = c["c"], c["sc"]
        g["sums"] = 3.0 * _rand((STAT_REPLICAS, 2, sc), seed).double() + 1e-9 * _rand((STAT_REPLICAS, 2, sc), seed + 1).double()
        g["save"] = torch.stack([0.1 * _rand((sc,), seed + 20), 1 + 0.2 * _rand((sc,), seed + 21).abs()]).contiguous()
        if "nogamma" not in f:
            g["gamma"] = 1 + 0.2 * _rand((ch,), seed + 60)
        if "nograd" not in f:
            g["dgamma0"], g["dbeta0"] = _rand((ch,), seed + 65), _rand((ch,), seed + 66)
    elif op == "fold":
        g["stats"] = (_rand((c["nrep"], c["n"]), seed).double() * 1e3 + _rand((c["nrep"], c["n"]), seed + 1).double() * 1e-6)
    else:
        g["part"] = _rand((c["nrep"], c["n"]), seed)
    return g


def inputs(name, seed=7):
    """Seeded inputs; a seed at which some activation input changes sign between float32 and float64 is passed over."""
    for s in range(seed, seed + 1000, 100):
        g = _gen(name, s)
        if "ytab" not in g or _kinks(g["y"], g["ytab"]) == 0:
            return g
    raise AssertionError(f"{name}: no seed without an activation kink")


def bwd_count(c):
    return 416.0 if c["op"] == "bwd_finalize" else float(c["n"] * c["h"] * c["w"])


# ---------------------------------------------------------------- kernels
def _to(g, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in g.items()}


def _coef_out(out, coef, coff, ch, pre):
    t = coef[:, coff:coff + ch].cpu().numpy()
    out[pre + "A"], out[pre + "B"], out[pre + "C"] = t[0], t[1], t[2]
    out[pre + "outside_ok"] = np.array(bool((_outside(coef, coff, ch) == PREFILL).all()))


def _run_reduce(name, dev, g, expect_fail, fin_separate=True):
    c = _ALL[name]
    f, ch, cs, coff = c["flags"], c["c"], c["cs"], c["coff"]
    d = _to(g, dev)
    L, st = _lib.lib(), _lib.stream()
    y, dz = d["y"].clone(), d["dz"].clone()
    vy = _view(y, coff, ch, d.get("ytab"), d.get("ygate"))
    gv = GradView()
    gv.dz, gv.dpool, gv.coef = dz.data_ptr(), (d["dpool"].data_ptr() if "dpool" in d else None), None
    sums = torch.zeros(STAT_REPLICAS * 2 * ch + STAT_PAD, dtype=torch.float64, device=dev)
    fin, fb = None, {}
    if "fin" in f:
        fcs, fcoff, fc = c.get("fin_slice", (cs, coff, ch))
        fb = {"counter": torch.zeros(TICKET_WORDS, dtype=torch.int32, device=dev), "coef": torch.full((3, max(cs, fcs)), PREFILL, device=dev),
              "dgamma": d["dgamma0"].clone(), "dbeta": d["dbeta0"].clone()}
        fin = BnBwdFin()
        fin.counter, fin.gamma, fin.coef = fb["counter"].data_ptr(), d["gamma"].data_ptr(), fb["coef"].data_ptr()
        fin.dgamma, fin.dbeta, fin.count = fb["dgamma"].data_ptr(), fb["dbeta"].data_ptr(), bwd_count(c)
        fin.cstride, fin.coff, fin.C = fcs, fcoff, fc
    rc = L.lhn_bn_bwd_reduce(C.byref(vy), C.byref(gv), _lib.ptr(d["save"]), _lib.ptr(sums), C.byref(fin) if fin is not None else None, st)
    torch.cuda.synchronize()
    if expect_fail:
        return rc, bool((sums == 0).all()) and bool((fb["coef"] == PREFILL).all()) and bool((fb["counter"] == 0).all()) and \
            torch.equal(fb["dgamma"], d["dgamma0"]) and torch.equal(fb["dbeta"], d["dbeta0"])
    _lib.check(rc, f"bn bwd reduce {name}")
    tot = sums[:STAT_REPLICAS * 2 * ch].view(STAT_REPLICAS, 2, ch).cpu().numpy().sum(0)      # replicas folded on the host, float64
    out = {"sums_du": tot[0], "sums_duxhat": tot[1], "sums_pad_ok": np.array(bool((sums[STAT_REPLICAS * 2 * ch:] == 0).all())),
           "inputs_ok": np.array(torch.equal(y, d["y"]) and torch.equal(dz, d["dz"]))}
    if fin is not None:
        _coef_out(out, fb["coef"], coff, ch, "coef_")
        out["dgamma"], out["dbeta"] = fb["dgamma"].cpu().numpy(), fb["dbeta"].cpu().numpy()
        if fin_separate:
            c2, dg2, db2 = torch.full((3, cs), PREFILL, device=dev), d["dgamma0"].clone(), d["dbeta0"].clone()
            _lib.check(L.lhn_bn_bwd_finalize2(_lib.ptr(sums), _lib.ptr(d["gamma"]), _lib.ptr(d["save"]), _lib.ptr(c2), cs, coff, ch, ch,
                                              C.c_double(bwd_count(c)), _lib.ptr(dg2), _lib.ptr(db2), C.c_float(1.0), st), "bn bwd finalize")
            torch.cuda.synchronize()
            out["sep_bits_equal"] = np.array(torch.equal(c2, fb["coef"][:, :cs]) and torch.equal(dg2, fb["dgamma"]) and torch.equal(db2, fb["dbeta"]))
            t = c2[:, coff:coff + ch].cpu().numpy()
            out["sep_coef_A"], out["sep_coef_B"], out["sep_coef_C"] = t[0], t[1], t[2]
            out["sep_dgamma"], out["sep_dbeta"] = dg2.cpu().numpy(), db2.cpu().numpy()
    return out


def _run_finalize(name, dev, g):
    c = _ALL[name]
    f, ch, sc, cs, coff = c["flags"], c["c"], c["sc"], c["cs"], c["coff"]
    d = _to(g, dev)
    L, st = _lib.lib(), _lib.stream()
    train, run_stats = "eval" not in f, "norun" not in f
    sbuf = torch.cat([d["stats"].reshape(-1), torch.full((STAT_PAD,), PREFILL, dtype=torch.float64, device=dev)])
    before = sbuf.clone()
    table, save = torch.full((3, cs), PREFILL, device=dev), torch.full((2, sc), PREFILL, device=dev)
    rm, rv, nbt = d["rmean"].clone(), d["rvar"].clone(), torch.full((1,), 5, dtype=torch.int64, device=dev)
    _lib.check(L.lhn_bn_finalize2(_lib.ptr(sbuf), _lib.ptr(d.get("gamma")), _lib.ptr(d.get("beta")), _lib.ptr(rm if run_stats else None),
                                  _lib.ptr(rv if run_stats else None), _lib.ptr(nbt), _lib.ptr(table), cs, coff, ch, sc, _lib.ptr(save),
                                  C.c_double(g["x"].shape[0]), C.c_float(EPS), C.c_float(MOMENTUM), C.c_float(SLOPE), int(train),
                                  _lib.ptr(d.get("cbias")), st), f"bn finalize {name}")
    torch.cuda.synchronize()
    t = table[:, coff:coff + ch].cpu().numpy()
    out = {"scale": t[0], "shift": t[1], "slope": t[2], "table_outside_ok": np.array(bool((_outside(table, coff, ch) == PREFILL).all())),
           "stats_ok": np.array(torch.equal(sbuf, before)), "nbt": nbt.cpu().numpy()}
    if train:
        out["mean"], out["invstd"] = save[0, :ch].cpu().numpy(), save[1, :ch].cpu().numpy()
        out["save_pad_ok"] = np.array(bool((save[:, ch:] == PREFILL).all()))
        if run_stats:
            out["rmean"], out["rvar"] = rm.cpu().numpy(), rv.cpu().numpy()
        else:
            out["running_ok"] = np.array(torch.equal(rm, d["rmean"]) and torch.equal(rv, d["rvar"]))
    else:
        out["save_pad_ok"] = np.array(bool((save == PREFILL).all()))
        out["running_ok"] = np.array(torch.equal(rm, d["rmean"]) and torch.equal(rv, d["rvar"]))
    return out


def _run_bwd_finalize(name, dev, g):
    c = _ALL[name]
    f, ch, sc, cs, coff = c["flags"], c["c"], c["sc"], c["cs"], c["coff"]
    d = _to(g, dev)
    L, st = _lib.lib(), _lib.stream()
    sbuf = torch.cat([d["sums"].reshape(-1), torch.full((STAT_PAD,), PREFILL, dtype=torch.float64, device=dev)])
    before = sbuf.clone()
    coef = torch.full((3, cs), PREFILL, device=dev)
    dg, db = (d["dgamma0"].clone(), d["dbeta0"].clone()) if "dgamma0" in d else (None, None)
    _lib.check(L.lhn_bn_bwd_finalize2(_lib.ptr(sbuf), _lib.ptr(d.get("gamma")), _lib.ptr(d["save"]), _lib.ptr(coef), cs, coff, ch, sc,
                                      C.c_double(bwd_count(c)), _lib.ptr(dg), _lib.ptr(db), C.c_float(0.5 if "pgrad" in f else 1.0), st),
               f"bn bwd finalize {name}")
    torch.cuda.synchronize()
    out = {"sums_ok": np.array(torch.equal(sbuf, before))}
    _coef_out(out, coef, coff, ch, "coef_")
    if dg is not None:
        out["dgamma"], out["dbeta"] = dg.cpu().numpy(), db.cpu().numpy()
    return out


def _run_fold(name, dev, g):
    c = _ALL[name]
    n, nrep = c["n"], c["nrep"]
    L, st = _lib.lib(), _lib.stream()
    buf = torch.cat([g["stats"].reshape(-1), torch.full((STAT_PAD,), PREFILL, dtype=torch.float64)]).to(dev)
    _lib.check(L.lhn_fold_stat_replicas(_lib.ptr(buf), C.c_int64(n), nrep, st), f"fold {name}")
    torch.cuda.synchronize()
    return {"rep0": buf[:n].cpu().numpy(), "others_zero_ok": np.array(bool((buf[n:nrep * n] == 0).all())),
            "pad_ok": np.array(bool((buf[nrep * n:] == PREFILL).all()))}


def _run_repl(name, dev, g, expect_fail):
    c = _ALL[name]
    n, nrep, alias = c["n"], c["nrep"], "alias" in c["flags"]
    rs = (n + 3) // 4 * 4 + 8
    L, st = _lib.lib(), _lib.stream()
    part = torch.full((nrep, rs), PREFILL, device=dev)
    part[:, :n] = g["part"].to(dev)
    before = part.clone()
    out_t = part if alias else torch.full((n + 8,), PREFILL, device=dev)
    rc = L.lhn_reduce_replicas(_lib.ptr(out_t), _lib.ptr(part), C.c_int64(n), nrep, C.c_int64(rs), st)
    torch.cuda.synchronize()
    if expect_fail:
        return rc, torch.equal(part, before) and bool((out_t.reshape(-1)[n:n + 8] == PREFILL).all()) and (alias or bool((out_t == PREFILL).all()))
    _lib.check(rc, f"reduce replicas {name}")
    out = {"out": out_t.reshape(-1)[:n].cpu().numpy()}
    if alias:
        out["others_ok"] = np.array(torch.equal(part[1:], before[1:]) and bool((part[0, n:] == PREFILL).all()))
    else:
        out["others_ok"] = np.array(torch.equal(part, before) and bool((out_t[n:] == PREFILL).all()))
    return out


def run(name, dev, g=None, expect_fail=False, **kw):
    """Outputs of a case as numpy arrays, plus `*_ok` flags: every float outside the outputs (the STAT_PAD doubles behind each
    statistics array, table / coef / save columns outside the slice, the inputs) still holds its bits."""
    g = g or inputs(name)
    op = _ALL[name]["op"]
    if op == "reduce":
        return _run_reduce(name, dev, g, expect_fail, **kw)
    if op == "repl":
        return _run_repl(name, dev, g, expect_fail)
    return {"finalize": _run_finalize, "bwd_finalize": _run_bwd_finalize, "fold": _run_fold}[op](name, dev, g)


# ---------------------------------------------------------------- reference
def _coef_ref(out, db, dg, gamma, mean, inv, count, pre):
    s = gamma * inv
    out[pre + "A"], out[pre + "B"] = s.double().numpy(), (-s * inv * dg / count).double().numpy()
    out[pre + "C"] = (-s * db / count + s * inv * mean * dg / count).double().numpy()


def reference(name, g=None, dtype=torch.float64):
    c = _ALL[name]
    f, op = c["flags"], c["op"]
    g = g or inputs(name)
    out = {}
    if op == "reduce":
        n, h, w, ch = c["n"], c["h"], c["w"], c["c"]
        ys = slice(c["coff"], c["coff"] + ch)
        e = g["dz"][..., ys].to(dtype)
        if "ygate" in g:
            e = e * g["ygate"][:, ys].to(dtype)[:, None, None, :]
        if "dpool" in g:
            slot = torch.tensor([[_seg(i, h) * 5 + _seg(j, w) for j in range(w)] for i in range(h)])
            e = e + g["dpool"][:, :, ys].to(dtype)[:, slot.view(-1)].view(n, h, w, ch)
        du = e * _dact(g["y"][..., ys], g["ytab"][:, ys], dtype) if "ytab" in g else e
        mean, inv = g["save"][0].to(dtype), g["save"][1].to(dtype)
        db, dg = du.sum((0, 1, 2)), (du * ((g["y"][..., ys].to(dtype) - mean) * inv)).sum((0, 1, 2))
        out["sums_du"], out["sums_duxhat"] = db.double().numpy(), dg.double().numpy()
        if "fin" in f:
            _coef_ref(out, db, dg, g["gamma"].to(dtype), mean, inv, bwd_count(c), "coef_")
            out["dgamma"], out["dbeta"] = (g["dgamma0"].to(dtype) + dg).double().numpy(), (g["dbeta0"].to(dtype) + db).double().numpy()
    elif op == "finalize":
        ch = c["c"]
        x = g["x"][:, :ch].to(dtype)
        cnt = x.shape[0]
        gamma = g["gamma"].to(dtype) if "gamma" in g else torch.ones(ch, dtype=dtype)
        beta = g["beta"].to(dtype) if "beta" in g else torch.zeros(ch, dtype=dtype)
        cb = g["cbias"].to(dtype) if "cbias" in g else torch.zeros(ch, dtype=dtype)
        if "eval" in f:
            mean, var = g["rmean"].to(dtype) - cb, g["rvar"].to(dtype)
        else:
            mean, var = x.mean(0), x.var(0, unbiased=False)
        invstd = 1.0 / torch.sqrt(var + EPS)
        scale = gamma * invstd
        out["scale"], out["shift"] = scale.double().numpy(), (beta - mean * scale).double().numpy()
        out["slope"] = np.full(ch, np.float32(SLOPE), np.float64)
        if "eval" not in f:
            out["mean"], out["invstd"] = mean.double().numpy(), invstd.double().numpy()
            if "norun" not in f:
                unb = var * cnt / (cnt - 1) if cnt > 1 else var           # one pixel: the library keeps the biased variance (torch refuses)
                out["rmean"] = ((1 - MOMENTUM) * g["rmean"].to(dtype) + MOMENTUM * (mean + cb)).double().numpy()
                out["rvar"] = ((1 - MOMENTUM) * g["rvar"].to(dtype) + MOMENTUM * unb).double().numpy()
    elif op == "bwd_finalize":
        ch = c["c"]
        tot = g["sums"].to(dtype).sum(0)[:, :ch]
        gamma = g["gamma"].to(dtype) if "gamma" in g else torch.ones(ch, dtype=dtype)
        _coef_ref(out, tot[0], tot[1], gamma, g["save"][0, :ch].to(dtype), g["save"][1, :ch].to(dtype), bwd_count(c), "coef_")
        if "dgamma0" in g:
            ps = 0.5 if "pgrad" in f else 1.0
            out["dgamma"], out["dbeta"] = (g["dgamma0"].to(dtype) + ps * tot[1]).double().numpy(), (g["dbeta0"].to(dtype) + ps * tot[0]).double().numpy()
    else:                                   # fold / repl: the replicas added in order r = 0, 1, .., in the given precision
        src = (g["stats"] if op == "fold" else g["part"]).to(dtype).numpy()
        s = src[0].copy()
        for r in range(1, c["nrep"]):
            s = s + src[r]
        out["rep0" if op == "fold" else "out"] = s
    return out


def exact(name, g=None):
    """What the kernel must give bit for bit: fold: the sequential float64 sum; repl: the sequential float32 sum."""
    op = _ALL[name]["op"]
    r = reference(name, g, torch.float64 if op == "fold" else torch.float32)
    return r["rep0"] if op == "fold" else r["out"].astype(np.float32)


def _check_reference():
    import time
    t0, worst = time.time(), 0.0
    for nm, c in CASES.items():
        g = inputs(nm)
        assert g["seed"] == 7, f"{nm} needed seed {g['seed']}"
        assert "ytab" not in g or _kinks(g["y"], g["ytab"]) == 0
        r64, r32 = reference(nm, g), reference(nm, g, torch.float32)
        for k in r64:
            assert np.isfinite(r64[k]).all() and np.abs(r64[k]).max() > 0, f"{nm} {k}: reference not finite or all zeros"
            e = rel_err(r32[k], r64[k])
            assert np.isfinite(3 * e), f"{nm} {k}"
            worst = max(worst, e)
        if "const" in c["flags"]:
            assert abs(r64["invstd"][3] - EPS ** -0.5) < 1e-9 and r64["mean"][3] == float(np.float32(1.7)), nm
        print(f"{nm:14s} {kernel_of(nm)}")
    for nm in ("r_c20", "r_c40", "r_c256", "r_c320", "r_c1024"):
        assert "LDS fold" in kernel_of(nm), nm
    for nm in ("r_c32", "r_c64_view", "r_c128_w37", "r_c16", "r_c4", "r_w3", "r_rows"):
        assert "shuffle" in kernel_of(nm), nm
    print(f"{len(CASES)} cases, no activation kinks at seed 7, worst float32 error {worst:.2e}, {time.time() - t0:.1f} s")


if __name__ == "__main__":
    if sys.argv[1] == "--check-reference":
        _check_reference()
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
