"""CPU: which gate-gradient pass a training plan leaves to the head's backward (lhn_gatesum) -- no GPU, no kernel launch.

The decision is taken by the plan EXECUTOR (csrc/lhn_plan.cpp: head_gate_fold_at, asked here through lhn_plan_head_gate_fold), not by
a pass of the plan compiler: tests/plan_digests.json pins the op lists of every variant byte for byte, and a compiler pass would
have changed the backward list of every configuration of B.  The op lists are therefore the same with the switch on and off (as
for LHN_BWD_FIN_CONSUMER); what changes is that a whole-plan run does not launch the GATE_REDUCE op the function names and hands its
slots (dgate | T0 | T1, the slices' saved statistics) to the PW_BWD op in front of it.

Variant B at 64x64: the head (128 -> 21, NCHW) is the only reader of neck[1]'s gated buffer; its PW_BWD stores the gradient of the
whole buffer and the GATE_REDUCE of that buffer follows directly: eight GATE_REDUCE ops in the list, seven launched.
Variants A and M: the head reads the output of a convolution + BatchNorm without a gate (the op after its PW_BWD is that BatchNorm's
BN_BWD), so nothing is folded; their heads still take the streaming forward and backward kernels (same 128 -> 21 shape).
LHN_HEAD_STREAM=0 or LHN_DETERMINISTIC=1 (both read once per process: child processes here): nothing is folded."""
import ctypes as C
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def probe(variant, size=64):
    """(index of the GATE_REDUCE op the run leaves out or -1, GATE_REDUCE ops in the list, the (kind, nchw, store mode, input buffer,
    whole buffer?) of the op in front of it, that GATE_REDUCE's (buffer, dgate offset, T0|T1 flag))."""
    from litehandnet_amd import _lib, get_model
    from litehandnet_amd.config import litehandnet_cfg
    from litehandnet_amd.plan import GATE_REDUCE, PlanBuilder
    cfg = litehandnet_cfg(variant, image_size=size)
    cfg.MODEL["ca_dropout"] = 0.0
    m = get_model(cfg)
    tensors = list(m.state_dict(keep_vars=True).values())
    pb = PlanBuilder(2, {id(t): j for j, t in enumerate(tensors)}, image_hw=(size, size), with_backward=True, p_drop=0.0)
    y = m.emit(pb, pb.image())
    if y.buf != -2:
        pb.set_output(y)
    cb, cf, cbw, nf, nb = pb.finalize()
    L = _lib.lib()
    L.lhn_plan_head_gate_fold.argtypes = [C.c_void_p]
    L.lhn_plan_head_gate_fold.restype = C.c_int
    h = L.lhn_plan_create(cb, len(pb.bufs), cf, nf, cbw, nb)
    assert h, L.lhn_last_error().decode()
    try:
        idx = L.lhn_plan_head_gate_fold(C.c_void_p(h))
    finally:
        L.lhn_plan_destroy(C.c_void_p(h))
    n_gate = sum(1 for j in range(nb) if cbw[j].kind == GATE_REDUCE)
    if idx < 0:
        return idx, n_gate, None, None
    p, q = cbw[idx - 1], cbw[idx]
    whole = p.in_coff[0] == 0 and p.in_C[0] == pb.bufs[p.in_buf[0]].C
    return idx, n_gate, (p.kind, p.i[1], p.i[2], p.in_buf[0], whole, p.in_C[0], p.out_C), (q.kind, q.out_buf, q.ws[3], q.ws[4])


def _child(variant, **env_extra):
    env = {k: v for k, v in os.environ.items() if k not in ("LHN_HEAD_STREAM", "LHN_DETERMINISTIC")}
    r = subprocess.run([sys.executable, os.path.abspath(__file__), variant], env=dict(env, **env_extra), capture_output=True, text=True,
                       timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    idx, n_gate = r.stdout.split()[-2:]
    return int(idx), int(n_gate)


def test_variant_b_leaves_one_gate_pass_to_the_head():
    from litehandnet_amd.plan import GATE_REDUCE, PW_BWD
    idx, n_gate = _child("B")
    assert n_gate == 8 and idx >= 1                      # eight in the list, this one not launched: seven k_gate_bwd_reduce per step
    if os.environ.get("LHN_HEAD_STREAM") != "0" and os.environ.get("LHN_DETERMINISTIC") != "1":
        idx2, n2, head, gate = probe("B")
        assert (idx2, n2) == (idx, n_gate)
        # the head's PW_BWD: NCHW, dx stored (mode 1), the whole 128-channel buffer, 21 features -- and the pass it takes over
        assert head == (PW_BWD, 1, 1, head[3], True, 128, 21)
        assert gate[0] == GATE_REDUCE and gate[1] == head[3] and gate[2] >= 0 and gate[3] >= 0


@pytest.mark.parametrize("env", [{"LHN_HEAD_STREAM": "0"}, {"LHN_DETERMINISTIC": "1"}])
def test_switch_off_or_deterministic_folds_nothing(env):
    assert _child("B", **env) == (-1, 8)


@pytest.mark.parametrize("variant", ["A", "M"])
def test_ungated_head_input_folds_nothing(variant):
    assert _child(variant) == (-1, 2)                    # (their two GATE_REDUCE ops belong to buffers the head does not read)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    res = probe(sys.argv[1])
    print(res[0], res[1])
