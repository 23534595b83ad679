"""The streaming kernels of the heatmap head (k_head_fwd / k_head_bwd in csrc/k_conv_head.hip: 128 -> <= 32 features, NCHW result),
called through the C ABI (lhn_conv_pw_fwd2, lhn_conv_pw_bwd5) and compared element by element with a float64 computation on the
CPU.  Inputs and references are those of tests/pw_cases.py; the cases below are added to its tables in memory.  x is channels
[64, 192) of a 192-channel buffer with a pending table and a gate, y_nchw / dy_nchw are stack 1 of 2.

Bar: the kernels before these (k_pw_fwd<128,1,1>, k_pw_bwd<128,1,true> + k_bias_grad_nchw, reached with LHN_HEAD_STREAM=0 in a child
process) run the same cases in the same session; for each output the new kernel's largest error against float64, relative to the
output's largest magnitude, may be at most twice theirs (the rule of tests/test_pw_bwd_narrow_gpu.py).

Pixel counts (forward tile 128 pixels, backward tile 64): 3 x 8x8 = one backward tile per image; 2 x 8x16 = two; 3 x 6x6 = H*W = 36,
tiles straddle images (the kernels take the gate per row there; with gate sums the launcher keeps the present kernels);
5 x 16x16 = 20 / 10 tiles; 1 x 10x10 = the last tile is partial (rows beyond M); 9 x 64x64 = 576 backward tiles, more than the 512
resident workgroups of a 256-CU device: the only case where a workgroup of the backward walks more than one tile outside
deterministic mode (under LHN_DETERMINISTIC=1 four workgroups share the 20 tiles of 5 x 16x16); 520 x 8x16 = the same for the gate
sums: 1,040 tiles in runs of three, two tiles per image, so the sums are carried across tiles and flushed at an image change in mid-run.

Gate sums (lhn_gatesum): dgate | T0 | T1 of x's buffer against float64, bar = twice the error of lhn_gate_bwd_reduce3 run on the
same (x, dx) -- the dx this call stored.  lhn_gate_bwd_reduce3 wants the whole buffer with its T0 | T1, so these cases run on a
128-channel buffer at offset 0 (the kernel indexes the sums by the channel in the buffer either way).

Known miss: dbias of head_gs2_runs (347 workgroups, 16 replicas) does not hold the factor-2 bar in every session.  Both kernels' dbias
carries about one float ulp of atomic-order rounding there, and the spread exceeds the factor: k_bias_grad_nchw measured 1.51e-7 and
6.09e-8 against float64 in two sessions (2.5x against itself), k_head_bwd 1.09e-7 and 1.22e-7; the first session passed (bar
3.02e-7), the second missed by 0.2 % (1.222e-7 against 1.219e-7).  The bar stays.  A bias gradient that holds it every time needs the
workgroups' double partials to meet before the one float rounding, i.e. a double scratch the entry point does not have.

Deterministic mode: the backward without gate sums runs there too (four workgroups, one writer per replica); two child runs agree
bit for bit.  With gate sums the call keeps the present kernels in that mode, so does the plan (tests/test_head_plan_cpu.py).

Run as a script it is the child: python tests/test_head_stream_gpu.py OUT.npz REPEATS NAME ...  (NAME = fwd:case | bwd:case)"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pw_cases as pc
from conftest import parity_record

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FACTOR = 2.0
PIXELS = {"one": (3, 8, 8), "two": (2, 8, 16), "straddle": (3, 6, 6), "multi": (5, 16, 16), "tail": (1, 10, 10)}
FWD_FLAGS, BWD_FLAGS = "xtab xgate xview nchw bias nostats", "nchw dbias xgate views"

FWD, BWD = {}, {}
for _tag, _nhw in PIXELS.items():
    FWD[f"head_fwd_{_tag}"] = pc._case(128, 21, _nhw, FWD_FLAGS)
    BWD[f"head_bwd_{_tag}"] = pc._case(128, 21, _nhw, BWD_FLAGS)                      # dx stored into its prefill, four replicas
for _co in (4, 32):                                                                     # the edges of the channel range
    FWD[f"head_fwd_c{_co}"] = pc._case(128, _co, PIXELS["two"], FWD_FLAGS)
    BWD[f"head_bwd_c{_co}"] = pc._case(128, _co, PIXELS["two"], BWD_FLAGS)
BWD["head_bwd_acc"] = pc._case(128, 21, PIXELS["tail"], BWD_FLAGS + " acc", nrep=1)     # dx added to a prior, one replica
BWD["head_bwd_nodx"] = pc._case(128, 21, PIXELS["two"], BWD_FLAGS + " nodx")
BWD["head_bwd_big"] = pc._case(128, 21, (9, 64, 64), BWD_FLAGS, nrep=16)
# gate sums: (BatchNorm slices as (first channel, channels), slope 0 on the first 64 channels of the table)
GS = {"head_gs0_one": (PIXELS["one"], (), False), "head_gs1_two": (PIXELS["two"], ((64, 64),), False),
      "head_gs2_multi": (PIXELS["multi"], ((0, 32), (64, 64)), True), "head_gs2_straddle": (PIXELS["straddle"], ((0, 32), (64, 64)), True)}
# 520 x 8x16 = 1,040 tiles of two per image, more than the 512 resident workgroups: runs of three consecutive tiles, so a workgroup
# carries its sums from tile to tile AND meets a new image inside its run (the flush on image change), at either position
GS["head_gs2_runs"] = ((520, 8, 16), ((0, 32), (64, 64)), True)
for _nm, (_nhw, _sl, _s0) in GS.items():
    BWD[_nm] = pc._case(128, 21, _nhw, "nchw dbias xgate", slices=_sl, slope0=_s0, **({"nrep": 16} if _nhw[0] > 100 else {}))
pc._ALL["fwd"].update(FWD)
pc._ALL["bwd"].update(BWD)
SMALL_BWD = [n for n in BWD if n != "head_bwd_big"]
DET = ["fwd:head_fwd_multi", "fwd:head_fwd_tail", "bwd:head_bwd_multi", "bwd:head_bwd_tail", "bwd:head_bwd_acc"]


class BnSlices(C.Structure):      # lhn_bn_slices (include/lhn.h)
    _fields_ = [("save", C.c_void_p * 2), ("sums", C.c_void_p * 2), ("lo", C.c_int32 * 2), ("C", C.c_int32 * 2), ("n", C.c_int32)]


class GateSum(C.Structure):       # lhn_gatesum
    _fields_ = [("dgate", C.c_void_p), ("slices", C.c_void_p)]


_IN = {}


def _inputs(kind, name):
    """pc.inputs plus, for a gate-sum case, the slices' saved statistics; the table's slope is 0 on half the channels if asked."""
    if (kind, name) not in _IN:
        g = pc.inputs(kind, name)
        c = pc._ALL[kind][name]
        if c.get("slope0"):
            g["xtab"][2, :64] = 0.0
        for k, (lo, cc) in enumerate(c.get("slices", ())):
            g[f"save{k}"] = torch.stack([0.1 * pc._rand((cc,), 70 + k), 1 + 0.2 * pc._rand((cc,), 80 + k).abs()]).contiguous()
        _IN[(kind, name)] = g
    return _IN[(kind, name)]


def _slices(c, d, keep):
    sl = BnSlices()
    for k, (lo, cc) in enumerate(c.get("slices", ())):
        sl.save[k], sl.lo[k], sl.C[k] = d[f"save{k}"].data_ptr(), lo, cc
    sl.n = len(c.get("slices", ()))
    keep.append(sl)
    return sl


def run_bwd(name, dev, g, with_gs=True, force_acc=False):
    """lhn_conv_pw_bwd5 on a case of BWD: dx, dW, dbias as pc.run_bwd returns them, `dy_ok` (dy keeps its bits), and for a gate-sum
    case gate = dgate | T0 | T1 as [3][N][C] plus the same from lhn_gate_bwd_reduce3 on the dx just stored (gate_reduce3).
    with_gs=False: the same call with the lhn_gatesum pointer NULL; gate is the (zeroed) arena as the call left it.
    force_acc: dx_accumulate = 1 whatever the case says; returns (status, dx and arena untouched?) for a call that must be refused."""
    c = BWD[name]
    f, (n, h, w), cin, cout = c["flags"], c["nhw"], c["cin"], c["cout"]
    xcs, xcoff, ycs, ycoff, ho, wo = pc.geometry("bwd", name)
    d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in g.items()}
    L, st = pc._lib.lib(), pc._lib.stream()
    vx = pc._view(d["x"], xcoff, cin, d["xtab"], d.get("xgate"))
    vy = pc._view(d["y"], ycoff, cout, d["ytab"])
    gv = pc.GradView()
    dy = d["dy_nchw"].clone()
    nrep = pc._nrep(c)
    rs = cout * cin + cout + 16
    gbuf = torch.zeros(nrep, rs, device=dev)
    dbp = C.c_void_p(gbuf.data_ptr() + 4 * cout * cin)
    if "nodx" in f:
        dx, acc = None, 0
    elif "prior" in d:
        dx, acc = d["prior"].clone(), 1
    else:
        dx, acc = torch.full((n, h, w, xcs), pc.PREFILL, device=dev), 0
    o = pc.PwOpts()
    o.nchw_batch_stride = pc.STACKS * cout * ho * wo
    keep, gsp, arena = [], None, None
    if "slices" in c:
        arena = torch.zeros(3, n, xcs, device=dev)
        gs = GateSum()
        gs.dgate, gs.slices = arena.data_ptr(), C.addressof(_slices(c, d, keep))
        keep.append(gs)
        gsp = C.byref(gs) if with_gs else None
    wdev = d["w"].contiguous()
    rc = L.lhn_conv_pw_bwd5(C.byref(vx), pc._lib.ptr(wdev), C.byref(vy), C.byref(gv), pc._lib.ptr(dx), 1 if force_acc else acc, pc._lib.ptr(gbuf), dbp, 1,
                            C.c_void_p(dy[:, 1].data_ptr()), nrep, C.c_int64(rs), C.byref(o), None, None, gsp, st)
    torch.cuda.synchronize()
    if force_acc:
        return rc, bool((dx == pc.PREFILL).all()) and not bool(arena.any()) and not bool(gbuf.any())
    pc._lib.check(rc, f"head bwd {name}")
    out = {"dy_ok": np.array(torch.equal(dy, d["dy_nchw"]))}
    tot = gbuf.sum(0)
    out["dw"] = tot[:cout * cin].view(cout, cin).cpu().numpy()
    out["dbias"] = tot[cout * cin:cout * cin + cout].cpu().numpy()
    out["dw_pad_ok"] = np.array(bool((gbuf[:, cout * cin + cout:] == 0).all()))
    if dx is not None:
        out["dx"] = dx[..., xcoff:xcoff + cin].cpu().numpy()
        before = d["prior"] if "prior" in d else torch.full_like(dx, pc.PREFILL)
        out["dx_outside_ok"] = np.array(torch.equal(pc._outside(dx, xcoff, cin), pc._outside(before, xcoff, cin)))
    if arena is not None:
        out["gate"] = arena.cpu().numpy()
    if arena is not None and with_gs:
        ref = torch.zeros(3, n, xcs, device=dev)
        vr = pc._view(d["x"], 0, xcs, d["xtab"])
        sl = _slices(c, d, keep)
        rc = L.lhn_gate_bwd_reduce3(C.byref(vr), pc._lib.ptr(dx), pc._lib.ptr(ref), C.c_void_p(ref.data_ptr() + 4 * n * xcs), C.byref(sl), 1, st)
        torch.cuda.synchronize()
        pc._lib.check(rc, f"gate reduce {name}")
        out["gate_reduce3"] = ref.cpu().numpy()
    return out


def reference_gate(name, g):
    """dgate | T0 | T1 in float64 from the float64 dx: [3][N][C]."""
    c = BWD[name]
    n, h, w = c["nhw"]
    dt = torch.float64
    dy = g["dy_nchw"][:, 1].to(dt).permute(0, 2, 1).reshape(-1, c["cout"])
    dx = (dy @ g["w"].to(dt)).view(n, h * w, 128)
    raw = g["x"].to(dt).view(n, h * w, 128)
    a = pc._value(g["x"], g["xtab"], None, dt).view(n, h * w, 128)
    da = pc._dact(g["x"], g["xtab"], dt).view(n, h * w, 128)
    mean, inv = torch.zeros(128, dtype=dt), torch.ones(128, dtype=dt)
    for k, (lo, cc) in enumerate(c["slices"]):
        mean[lo:lo + cc], inv[lo:lo + cc] = g[f"save{k}"][0].to(dt), g[f"save{k}"][1].to(dt)
    t = torch.stack([(dx * da).sum(1), (dx * da * (raw - mean) * inv).sum(1)], 1)        # [N][2][C]
    return torch.cat([(dx * a).sum(1).reshape(-1), t.reshape(-1)]).view(3, n, 128).numpy()


def _child(tmp, env_extra, names, reps=1):
    out = os.path.join(str(tmp), "out.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("LHN_HEAD_STREAM", "LHN_DETERMINISTIC")}
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out, str(reps)] + names, env=dict(env, **env_extra),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return dict(np.load(out))


def _of(res, full, rep=0):
    pre = f"{full}/{rep}/"
    return {k[len(pre):]: v for k, v in res.items() if k.startswith(pre)}


@pytest.fixture(scope="module")
def old_runs(dev, tmp_path_factory):
    """Every case on the kernels before these (LHN_HEAD_STREAM=0), once per session."""
    return _child(tmp_path_factory.mktemp("head_old"), {"LHN_HEAD_STREAM": "0"}, [f"fwd:{n}" for n in FWD] + [f"bwd:{n}" for n in BWD])


def _compare(tag, got, old, r64, keys):
    bad = []
    for k in keys:
        if k not in r64:
            continue
        assert got[k].shape == r64[k].shape == old[k].shape, f"{tag} {k}: shapes {got[k].shape} {old[k].shape} {r64[k].shape}"
        e_new, e_old = pc.rel_err(got[k], r64[k]), pc.rel_err(old[k], r64[k])
        parity_record(f"head_stream/{tag}", **{f"{k}_err_new": e_new, f"{k}_err_old": e_old, f"{k}_bar": FACTOR * e_old})
        print(f"head_stream {tag} {k}: new {e_new:.3e}  old {e_old:.3e}  bar {FACTOR * e_old:.3e}")
        if not e_new <= FACTOR * e_old:
            bad.append(f"{k}: {e_new:.3e} > {FACTOR} x {e_old:.3e}")
    for k, v in got.items():
        if k.endswith("_ok") and not bool(v):
            bad.append(f"{k}: floats that must keep their bits changed")
    assert not bad, f"{tag}: " + "; ".join(bad)


@pytest.mark.parametrize("name", list(FWD))
def test_head_fwd_matches_float64(dev, old_runs, name):
    g = _inputs("fwd", name)
    got = pc.run_fwd(name, dev, g)
    assert "nchw_other_ok" in got                     # stack 0 of y_nchw and the NHWC buffer keep their prefill
    _compare(name, got, _of(old_runs, f"fwd:{name}"), pc.reference_fwd(name, g), ("y_nchw",))


@pytest.mark.parametrize("name", list(BWD))
def test_head_bwd_matches_float64(dev, old_runs, name):
    g = _inputs("bwd", name)
    got = run_bwd(name, dev, g)
    assert ("dx" in got) == ("nodx" not in BWD[name]["flags"]) and "dy_ok" in got
    _compare(name, got, _of(old_runs, f"bwd:{name}"), pc.reference_bwd(name, g), ("dx", "dw", "dbias"))


@pytest.mark.parametrize("name", list(GS))
def test_head_gate_sums_match_float64(dev, name):
    """dgate | T0 | T1 per element against float64; bar: twice the error of lhn_gate_bwd_reduce3 on the same (x, dx)."""
    g = _inputs("bwd", name)
    got = run_bwd(name, dev, g)
    r64 = reference_gate(name, g)
    for j, k in enumerate(("dgate", "T0", "T1")):
        e_new, e_old = pc.rel_err(got["gate"][j], r64[j]), pc.rel_err(got["gate_reduce3"][j], r64[j])
        parity_record(f"head_stream/{name}", **{f"{k}_err_new": e_new, f"{k}_err_reduce3": e_old, f"{k}_bar": FACTOR * e_old})
        print(f"head_stream {name} {k}: in the head's launch {e_new:.3e}  lhn_gate_bwd_reduce3 {e_old:.3e}  bar {FACTOR * e_old:.3e}")
        assert e_new <= FACTOR * e_old, f"{name} {k}: {e_new:.3e} > {FACTOR} x {e_old:.3e}"
    if BWD[name]["slope0"]:
        assert not got["gate"][1][:, :64][r64[1][:, :64] == 0].any()      # slope 0 where u <= 0: those terms are exactly zero


def test_head_gate_sums_null_leaves_the_arena(dev):
    """The lhn_gatesum pointer NULL: the arena keeps its zeros, and dx, dW, dbias have the bits of the call with sums (the sums only
    read the accumulators)."""
    name = "head_gs1_two"
    g = _inputs("bwd", name)
    plain, full = run_bwd(name, dev, g, with_gs=False), run_bwd(name, dev, g)
    assert not plain["gate"].any() and full["gate"].any()
    for k in ("dx", "dw", "dbias"):
        np.testing.assert_array_equal(plain[k], full[k], err_msg=k)


def test_head_gate_sums_refuse_an_accumulated_dx(dev):
    """Gate sums with dx_accumulate: the head kernel would sum this call's part of dx, the reduce launch the whole buffer, so the
    call is refused on every route and writes nothing."""
    rc, untouched = run_bwd("head_gs1_two", dev, _inputs("bwd", "head_gs1_two"), force_acc=True)
    assert rc != 0 and "stored dx" in pc._lib.lib().lhn_last_error().decode() and untouched


def test_head_stream_switch_takes_the_old_path(dev, old_runs, tmp_path):
    """LHN_HEAD_STREAM=0: the kernels before these still answer (the float64 bar of tests/test_pw_gpu.py), and they are visibly
    other kernels.  At 9 x 64x64 the present backward runs 256 workgroups (one per CU) that take tiles b, b + 256, b + 512 into one
    accumulator, the new one 288 workgroups with two consecutive tiles each: another association of the same 576 terms in each of
    the 2,688 elements of dW, so its bits differ.  dbias differs everywhere: k_bias_grad_nchw sums in double."""
    name = "head_bwd_big"
    g = _inputs("bwd", name)
    r64, r32 = pc.reference_bwd(name, g), pc.reference_bwd(name, g, torch.float32)
    old = _of(old_runs, f"bwd:{name}")
    for k in ("dx", "dw", "dbias"):
        assert pc.rel_err(old[k], r64[k]) <= max(2e-5, 3 * pc.rel_err(r32[k], r64[k])), f"LHN_HEAD_STREAM=0 {name} {k}"
    got = _of(_child(tmp_path, {}, [f"bwd:{name}"]), f"bwd:{name}")        # a fresh process without the switch
    assert got["dw"].shape == old["dw"].shape and not np.array_equal(got["dw"], old["dw"]), f"{name}: the switch did not change the kernel"
    assert not np.array_equal(got["dbias"], old["dbias"]), f"{name}: dbias still comes from k_bias_grad_nchw"


def test_head_stream_deterministic(dev, tmp_path, old_runs):
    """LHN_DETERMINISTIC=1: the forward and the backward (without gate sums) run the streaming kernels with four workgroups, so a
    workgroup walks several tiles; two runs in two fresh processes agree bit for bit and meet the bar against the present kernels."""
    first = _child(tmp_path, {"LHN_DETERMINISTIC": "1"}, DET)
    second_dir = tmp_path / "second"
    second_dir.mkdir()
    second = _child(second_dir, {"LHN_DETERMINISTIC": "1"}, DET)
    for full in DET:
        kind, name = full.split(":")
        a, b = _of(first, full), _of(second, full)
        assert a and set(a) == set(b), full
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{full} {k}")
        g = _inputs(kind, name)
        _compare("deterministic/" + name, a, _of(old_runs, full), pc.reference(kind, name, g), ("y_nchw", "dx", "dw", "dbias"))


if __name__ == "__main__":
    dst, reps, names = sys.argv[1], int(sys.argv[2]), sys.argv[3:]
    device = torch.device("cuda:0")
    res = {}
    for full in names:
        knd, nm = full.split(":")
        inp = _inputs(knd, nm)
        for rep in range(reps):
            outs = pc.run_fwd(nm, device, inp) if knd == "fwd" else run_bwd(nm, device, inp)
            for key, val in outs.items():
                res[f"{full}/{rep}/{key}"] = val
    np.savez(dst, **res)
