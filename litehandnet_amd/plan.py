"""Static execution plan for the litehandnet backbone on one MI355X.

The reference runs ~330 unfused torch ops per forward.  Here the Python
mirror of the module tree (`liteHandNet.py`, `litehourglass.py`, ...) is walked ONCE per input
shape by a `PlanBuilder`; the result is a flat list of kernel calls over one workspace arena that
`lhn_plan_run` (csrc/lhn_plan.cpp) enqueues with a single C call per forward / backward.

Conventions
  * activations: NHWC fp32 buffers in the arena, each with a per-channel table (scale, shift,
    slope) and optionally a per-(n,c) gate; a conv writes its RAW output plus BatchNorm statistics,
    `FINALIZE` turns the statistics into the table, consumers apply it on load (no BN/act pass).
  * cat / chunk / channel slices are (buffer, coff, C) views -- producers write into slices.
  * gradients: one grad buffer per activation buffer holding d(loss)/d(consumed value); the
    backward list is generated here by walking the forward records in reverse and tracking which
    channel ranges have been written (store) or must be accumulated.
"""
import ctypes as C
import os
from dataclasses import dataclass, field

import torch

from . import _lib
from ._lib import Buf, Op

# op kinds (must match csrc/lhn_plan.cpp)
STEM, PW, DW, KXK, FINALIZE, EW, MAXPOOL, AVGPOOL, CA_MLP, TABLE_FILL, MEMSET, ATT_MLP, SE_MLP, SHUFFLE = range(1, 15)
PWDW = 15              # inference plans only: 1x1 -> depthwise 3x3 in one launch (lhn_conv_pw_dw3_fwd), see PlanBuilder.fuse_pw_dw
DWPW = 16              # inference plans only: depthwise 3x3 -> 1x1 in one launch (lhn_conv_dw3_pw_fwd), see PlanBuilder.fuse_dw_pw
MSRB = 17              # inference plans only: both depthwise branches of an MSRB round (+ its attention's pooling) in one pass
                       # (lhn_msrb_round_fwd), see PlanBuilder.fuse_msrb_round
CBAM = 18              # the CBAM chain between its `pre` convolutions and its final ReLU (lhn_cbam_fwd), see PlanBuilder.cbam_attention
BNECK = 19             # inference plans only: BottleNeck (1x1 -> 3x3 -> 1x1 + residual + activation) in one launch (lhn_bottleneck_fwd),
                       # see PlanBuilder.fuse_bottleneck
STEMTAIL = 20          # inference plans only: the stem after its first convolution (depthwise K x K, 1x1, 3x3 stride 2, max pool, 1x1) in one
                       # launch (lhn_stem_tail_fwd), see PlanBuilder.fuse_stem
CCW_POOL, CCW_GATE, CCW_DW, CCW_SHUFFLE = 21, 22, 23, 24   # inference plans only: a ConditionalChannelWeighting block of Lite-HRNet as four launches, each
                       # over all 2..4 branches (lhn_ccw_pool_fwd / _gate_fwd / _dw_fwd / _shuffle_fwd), see PlanBuilder.fuse_ccw
CCW_ARG = 25           # ... and the description of one branch (views and parameters) in front of the launches that read it: launches nothing
STEM_BWD, PW_BWD, DW_BWD, KXK_BWD, BN_BWD, EW_BWD, MAXPOOL_BWD, AVGPOOL_BWD, GATE_REDUCE, CA_MLP_BWD, ATT_MLP_BWD, SE_MLP_BWD, SHUFFLE_BWD = range(101, 114)
CBAM_BWD = 114
SLOPE_SILU = 2.0       # LHN_SLOPE_SILU in include/lhn.h: the combine applies SiLU instead of a leaky ReLU
SLOPE_RELU_SIGMOID = 3.0   # LHN_SLOPE_RELU_SIGMOID: sigmoid(relu(v)) (lite_hrnet.py: nn.ReLU followed by nn.Sigmoid)
EW_MUL, EW_BILINEAR = 1, 2   # EwSrcs.mode bits: product of the sources / bilinear (align_corners) resampling of smaller ones

ALIGN = 256
STAT_REPLICAS = 32     # LHN_STAT_REPLICAS in include/lhn.h
TICKET_WORDS = 33      # arrival counters of a fused finalize (lhn_bnfin.counter: one top word + 32 group words)


# Plan switches: every one is on by default and NAME=0 in the environment turns it off.  They are read at every plan build (the
# first two while the modules emit their records, the rest in finalize()), not once per process like the library's own.
PLAN_SWITCHES = {
    "LHN_COPY_POOL": "a gated RepBasicUnit's pass-through copy rides in the attention's pooling launch",
    "LHN_GATE_BN_SUMS": "BatchNorm-backward sums of gated buffers come from the attention's backward",
    "LHN_SUM_OUT": "the readers of a lazy residual sum also write it (no re-materialising combine in the backward)",
    "LHN_GRAD_ADDENDS": "depthwise backward kernels add the gradient of a residual sum while storing dx",
    "LHN_FUSE_BN_SUMS": "a producer's BatchNorm-backward sums ride in its only reader, a 3x3 depthwise backward",
    "LHN_READER_BN_SUMS": "... or in all of its readers' backward kernels (combines, pools, the fused 1x1 backward)",
    "LHN_POOL_GRAD_ADDS": "the max-pool backward also stores the gradients of the average pool and sum that read the same view",
    "LHN_EW_BWD_MULTI": "same-resolution sources of a combine get their gradients in one launch",
}


def _switch(name):
    """State of a plan switch, read from the environment now."""
    assert name in PLAN_SWITCHES, name
    return os.environ.get(name, "1") != "0"


# Inference switches: opt-in rewrites of plans without a backward.  One row per switch, in the order finalize() runs the passes:
# (PlanBuilder attribute and keyword, environment variable, pass method, counter attribute, what the pass does).  Every one is off
# unless NAME=1 is in the environment or its set_* function below switched it on in the process.  PlanBuilder's keywords differ in
# their defaults, and tests rely on it: infer_fuse, infer_fuse_dwpw and infer_fuse_msrb default to None = follow the process switch,
# infer_fuse_bneck, infer_bf16x3, infer_fuse_stem and infer_fuse_ccw to False (Engine.plan_for passes all seven).
INFER_SWITCHES = (
    ("infer_fuse_stem", "LHN_INFER_FUSE_STEM", "fuse_stem", "n_fused_stem", "the stem after its first convolution is one launch"),
    ("infer_fuse_msrb", "LHN_INFER_FUSE_MSRB", "fuse_msrb_round", "n_fused_msrb", "an MSRB round and its attention's pooling are one pass"),
    ("infer_fuse_dwpw", "LHN_INFER_FUSE_DWPW", "fuse_dw_pw", "n_fused_dwpw", "DWConv's depthwise 3x3 -> 1x1 is one launch"),
    ("infer_fuse", "LHN_INFER_FUSE", "fuse_pw_dw", "n_fused", "RepBasicUnit's 1x1 -> depthwise 3x3 is one launch"),
    ("infer_fuse_bneck", "LHN_INFER_FUSE_BNECK", "fuse_bottleneck", "n_fused_bneck", "a BottleNeck is one launch"),
    ("infer_bf16x3", "LHN_INFER_BF16X3", "mark_bf16x3", "n_bf16x3", "dense 3x3 convolutions run on the split-bf16 MFMA"),
    ("infer_fuse_ccw", "LHN_INFER_FUSE_CCW", "fuse_ccw", "n_fused_ccw", "a Lite-HRNet channel-weighting block is four grouped launches"),
)
_INFER_ENV = {row[0]: row[1] for row in INFER_SWITCHES}
_INFER_OVERRIDE = {}       # switch name -> bool: what _set_infer_switch put in front of the environment


def _infer_switch(name):
    """State of an inference switch now: the in-process override if there is one, else NAME=1 in the environment (default off)."""
    on = _INFER_OVERRIDE.get(name)
    return on if on is not None else os.environ.get(_INFER_ENV[name], "0") == "1"


def _set_infer_switch(name, on):
    """Switch an inference pass on or off for plans built from now on; None = follow the environment again.  The switches are
    independent of each other, and Engine.plan_for keys its cache on all of them, so the next forward builds the matching plan."""
    assert name in _INFER_ENV, name
    _INFER_OVERRIDE[name] = None if on is None else bool(on)


def set_infer_fuse(on):
    """_set_infer_switch for the 1x1 -> depthwise 3x3 inference fusion pass (PlanBuilder.fuse_pw_dw)."""
    _set_infer_switch("infer_fuse", on)


def infer_fuse_enabled():
    """LHN_INFER_FUSE=1 (default off): plans without a backward run RepBasicUnit's 1x1 -> depthwise 3x3 pairs as one launch."""
    return _infer_switch("infer_fuse")


def set_infer_fuse_dwpw(on):
    """_set_infer_switch for the depthwise -> 1x1 inference fusion pass (PlanBuilder.fuse_dw_pw)."""
    _set_infer_switch("infer_fuse_dwpw", on)


def infer_fuse_dwpw_enabled():
    """LHN_INFER_FUSE_DWPW=1 (default off): plans without a backward run DWConv's depthwise 3x3 -> 1x1 pairs as one launch."""
    return _infer_switch("infer_fuse_dwpw")


def set_infer_fuse_msrb(on):
    """_set_infer_switch for the MSRB-round inference fusion pass (PlanBuilder.fuse_msrb_round)."""
    _set_infer_switch("infer_fuse_msrb", on)


def infer_fuse_msrb_enabled():
    """LHN_INFER_FUSE_MSRB=1 (default off): plans without a backward run each MSRB round -- its two dilated depthwise 3x3
    convolutions and the pooling of its attention -- as one pass over the feature map."""
    return _infer_switch("infer_fuse_msrb")


def set_infer_fuse_bneck(on):
    """_set_infer_switch for the BottleNeck inference fusion pass (PlanBuilder.fuse_bottleneck)."""
    _set_infer_switch("infer_fuse_bneck", on)


def infer_fuse_bneck_enabled():
    """LHN_INFER_FUSE_BNECK=1 (default off): plans without a backward run each BottleNeck -- 1x1, dense 3x3, 1x1, residual sum and
    activation -- as one launch."""
    return _infer_switch("infer_fuse_bneck")


def set_infer_fuse_stem(on):
    """_set_infer_switch for the stem inference fusion pass (PlanBuilder.fuse_stem)."""
    _set_infer_switch("infer_fuse_stem", on)


def infer_fuse_stem_enabled():
    """LHN_INFER_FUSE_STEM=1 (default off): plans without a backward run the stem after its first convolution -- depthwise K x K, 1x1,
    dense 3x3 stride 2, max pool, concatenation and 1x1 -- as one launch."""
    return _infer_switch("infer_fuse_stem")


def set_infer_bf16x3(on):
    """_set_infer_switch for the split-bf16 pass for dense 3x3 convolutions (PlanBuilder.mark_bf16x3)."""
    _set_infer_switch("infer_bf16x3", on)


def infer_bf16x3_enabled():
    """LHN_INFER_BF16X3=1 (default off): plans without a backward run their stride-1 dense 3x3 convolutions with 32 / 64 / 128
    channels on the bf16 MFMA with a three-term split (lhn_conv_kxk_fwd_bf16x3) instead of the fp32 MFMA."""
    return _infer_switch("infer_bf16x3")


def set_infer_fuse_ccw(on):
    """_set_infer_switch for the ConditionalChannelWeighting inference pass (PlanBuilder.fuse_ccw)."""
    _set_infer_switch("infer_fuse_ccw", on)


def infer_fuse_ccw_enabled():
    """LHN_INFER_FUSE_CCW=1 (default off): plans without a backward run each ConditionalChannelWeighting block of Lite-HRNet -- 22 / 28
    launches over 3 / 4 branches -- as four launches, each over all branches (PlanBuilder.FUSE_CCW_BRANCHES: two-branch blocks stay)."""
    return _infer_switch("infer_fuse_ccw")


# What lhn_conv_kxk_fwd_bf16x3 is built for (csrc/k_conv_kxk_bf16.hip: kxk_bf16x3_channels and the checks of the entry point) ...
BF16X3_CHANNELS = (32, 64, 128)
# ... and the (Cin, Cout) classes the pass leaves on the fp32 kernel all the same.  32 -> 32: in variant A these are the
# inner 3x3 of the BottleNecks, whose small split error the following BatchNorm scales up: with them on the bf16 MFMA the heat maps of A
# at 256 x 256 sit 1.5e-4 of their peak from float64 (bar 1e-4; 1.2e-5 ... 3.3e-5 without them), and they are launch-bound, not
# MFMA-bound, so nothing is lost.
BF16X3_LEFT_OUT = ((32, 32),)


def bf16x3_eligible(cin, cout, stride, overlap=False):
    """THE eligibility rule of the bf16x3 pass: a stride-1 dense 3x3 (pad 1) the entry point accepts -- Cin and Cout in
    BF16X3_CHANNELS, an output view that does not overlap its input's channels in the same buffer -- and whose channel class has not
    been taken out by measurement (BF16X3_LEFT_OUT).  Any map size."""
    return stride == 1 and cin in BF16X3_CHANNELS and cout in BF16X3_CHANNELS and not overlap and (cin, cout) not in BF16X3_LEFT_OUT


def _refs_in(v):
    """Every TRef inside a record value (views, concatenations, lists of views or of (view, coefficient) pairs)."""
    if isinstance(v, TRef):
        yield v
    elif isinstance(v, TCat):
        yield from v.parts
    elif isinstance(v, (list, tuple)):
        for u in v:
            yield from _refs_in(u)


def _overlaps(x, y):
    """True when the views x and y share channels of one buffer."""
    return y.buf == x.buf and x.coff < y.coff + y.C and y.coff < x.coff + x.C


def _biased_bn(r):
    """True when the convolution record r has a bias in front of a BatchNorm: the unfused convolution's own finalize folds it into the
    table's shift, a FINALIZE record does not."""
    return r["bn"] is not None and getattr(r["conv"], "bias", None) is not None


def _reads(rec):
    """The views a record's launch reads as data (an attention record reads and gates its own buffer: not listed)."""
    k = rec["op"]
    if k in (STEM, PW, DW, KXK, MAXPOOL, AVGPOOL):
        return [rec["x"]]
    return rec["srcs"] if k == EW else [rec["a"], rec["b"]] if k == SHUFFLE else [rec["p"], rec["r"]] if k == CBAM else []


def _al(n):
    return (n + ALIGN - 1) // ALIGN * ALIGN


@dataclass
class TRef:
    """A (buffer, channel-slice) view.  buf == -1 is the NCHW input image."""
    buf: int
    coff: int
    C: int
    H: int
    W: int


@dataclass
class TCat:
    """Channel concatenation of views that live in DIFFERENT buffers (same N, H, W) -- the result of a torch.cat whose
    operands are never copied together: RepBasicUnit's pass-through half stays where it is (litehourglass.py:74-77) and
    every whole-tensor consumer (max-pool, residual add, average pool) runs once per part."""
    parts: list

    @property
    def C(self):
        return sum(p.C for p in self.parts)

    @property
    def H(self):
        return self.parts[0].H

    @property
    def W(self):
        return self.parts[0].W


def _parts(x):
    return list(x.parts) if isinstance(x, TCat) else [x]


@dataclass
class _BufRec:
    H: int
    W: int
    C: int
    gate: bool = False
    coef: bool = False
    dpool: bool = False
    lazy: object = None      # the EW record of a sum that is taken ON LOAD by its consumers (never written in forward)
    fused: bool = False      # a tensor between the convolutions of a PWDW / DWPW / BNECK / STEMTAIL launch: a table, no data
    off: dict = field(default_factory=dict)


class _Arena:
    def __init__(self):
        self.size = 0

    def take(self, nbytes):
        off = self.size
        self.size += _al(nbytes)
        return off


class _IdentConv:
    weight = None
    bias = None


_IDENT = _IdentConv()


@dataclass
class _BwdFusions:
    """What the backward analyses of PlanBuilder._lower_backward decided, in the order they ran (each saw the ones above it),
    and below them the two trackers the emitters fill while they walk the records in reverse."""
    uses: dict                  # buffer -> records that read it (_reader_map)
    aliased: set                # buffers whose gradient buffer is their only reader's (_alias_gradients)
    pending_add: dict           # buffer -> [(id(sum record), the sum's output buffer, channel shift)] (_grad_addends)
    bns: dict                   # (id(reader record), buf, coff, C) -> ((sums, save) offsets, (producer's C, channel offset)) (_reader_bn_sums)
    fused_mp: dict = field(default_factory=dict)       # id(max-pool record) -> ((sum record, source index) | None, average-pool record | None)
    skip_ew_src: set = field(default_factory=set)      # (id(sum record), source index) handled by a max-pool backward
    skip_ap: set = field(default_factory=set)          # id(average-pool record) handled by a max-pool backward (_pool_grad_fusion)
    written: dict = field(default_factory=dict)        # buffer -> channel ranges of its gradient written so far (_grad_mode)
    materialised: set = field(default_factory=set)     # lazy sums the backward list has re-materialised so far

    def bns_of(self, q, t):
        """(ws pair, (C, coff)) of the BatchNorm sums reader record q adds for its input view t, or ((-1, -1), (0, 0))."""
        return self.bns.get((id(q), t.buf, t.coff, t.C), ((-1, -1), (0, 0)))


class PlanBuilder:
    _no_grad_buf = -1   # the image never needs a gradient

    def __init__(self, N, state_index, image_hw=None, with_backward=True, p_drop=0.0, infer_fuse=None, infer_fuse_dwpw=None,
                 infer_fuse_msrb=None, infer_fuse_bneck=False, infer_bf16x3=False, infer_fuse_stem=False, infer_fuse_ccw=False):
        self.N = N
        # The inference switches (INFER_SWITCHES): None = the process-wide switch.  The rewritten launches have no batch statistics,
        # so the caller passes False for a plan that will run train-mode BatchNorm under no_grad (Engine.plan_for).
        given = locals()
        for name, _, _, counter, _ in INFER_SWITCHES:
            setattr(self, name, _infer_switch(name) if given[name] is None else bool(given[name]))
            setattr(self, counter, 0)
        self.state_index = state_index      # id(tensor) -> index in the params array
        self.bufs = []
        self.recs = []                      # forward records (python dicts)
        self.with_backward = with_backward
        self.p_drop = p_drop
        self.image_hw = image_hw
        # arenas: zf = zeroed at the start of every forward, zb = zeroed at the start of every backward
        self.ar = {"zf": _Arena(), "zb": _Arena(), "mask": _Arena(), "misc": _Arena()}
        self.out_ref = None
        self.nchw_out_C = None
        self.nchw_stacks = 1
        self.in_ref = None

    # ------------------------------------------------------------------ declarations
    def image(self):
        H, W = self.image_hw
        return TRef(-1, 0, 3, H, W)

    def buffer(self, H, W, C):
        self.bufs.append(_BufRec(H, W, C))
        return len(self.bufs) - 1

    def new(self, H, W, C):
        return TRef(self.buffer(H, W, C), 0, C, H, W)

    def input_tensor(self, C, H, W):
        self.in_ref = self.new(H, W, C)
        return self.in_ref

    def slice(self, x, coff, C):
        if not (0 <= coff and coff + C <= x.C and coff % 4 == 0 and C % 4 == 0):
            raise _lib.LhnError(f"channel slice [{coff}:{coff + C}] of {x.C} channels: slices start and end on multiples of 4 "
                                "(the kernels move 4 channels per thread)")
        if isinstance(x, TCat):
            out, lo = [], 0
            for p in x.parts:
                a, b = max(coff, lo), min(coff + C, lo + p.C)
                if a < b:
                    out.append(TRef(p.buf, p.coff + a - lo, b - a, p.H, p.W))
                lo += p.C
            return out[0] if len(out) == 1 else TCat(out)
        return TRef(x.buf, x.coff + coff, C, x.H, x.W)

    def cat(self, xs):
        """torch.cat(xs, dim=1) without a copy."""
        parts = [p for x in xs for p in _parts(x)]
        assert all((p.H, p.W) == (parts[0].H, parts[0].W) for p in parts)
        return parts[0] if len(parts) == 1 else TCat(parts)

    def single(self, x):
        """A one-buffer view of x (convolutions and gates read ONE buffer): multi-part tensors are copied together."""
        return self.ew([x]) if isinstance(x, TCat) else x

    def owns_buffer(self, x):
        """True when x is the whole of an ungated buffer that is not the block's input (a gate attaches to a buffer)."""
        if isinstance(x, TCat):
            return False
        self.real(x)
        b = self.bufs[x.buf]
        return x.coff == 0 and x.C == b.C and not b.gate and not (self.in_ref is not None and x.buf == self.in_ref.buf)

    @staticmethod
    def _segments(tensors):
        """Channel ranges (lo, hi) on which every tensor of the list is ONE part."""
        cuts = set()
        for t in tensors:
            lo = 0
            for p in _parts(t):
                cuts.add(lo)
                lo += p.C
            cuts.add(lo)
        cuts = sorted(cuts)
        return list(zip(cuts[:-1], cuts[1:]))

    def _ws(self, arena, nbytes):
        return (arena, self.ar[arena].take(nbytes))

    def _p(self, t):
        return -1 if t is None else self.state_index[id(t)]

    def _p_bn(self, bn):
        """The five parameter slots of a BatchNorm."""
        return tuple(self._p(t) for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked))

    def _bn_ws(self, rec, C, out):
        """Statistics work areas of a convolution + BatchNorm record over C channels (bump-allocated: the order is part of the layout)."""
        rec["stats"] = self._ws("zf", STAT_REPLICAS * 2 * C * 8)
        rec["cnt"] = self._ws("zf", 4 * TICKET_WORDS)
        rec["save"] = self._ws("misc", 2 * C * 4)
        if self.with_backward:
            rec["sums"] = self._ws("zb", STAT_REPLICAS * 2 * C * 8)
            rec["bcnt"] = self._ws("zb", 4 * TICKET_WORDS)
            self.bufs[out.buf].coef = True

    # ------------------------------------------------------------------ forward emitters
    def conv(self, x, conv, bn=None, slope=1.0, out=None, nchw_out=False, stack=None, bn_repeat=1):
        """conv (+ train/eval BatchNorm + leaky slope as a pending transform).  Returns the output view.
        1x1 convolutions take any channel counts: views are padded to multiples of 4 (a 21-feature head is a 24-channel
        NHWC buffer whose last channels are exact zeros) and the library slices wide ones.  `stack = (i, S)`: the NCHW output
        is slot i of an [N, S, K, H, W] tensor (hourglassnet.py:136)."""
        x = self.single(x)
        cout, cin_g, kh, kw = conv.weight.shape
        s, p, d, g = conv.stride[0], conv.padding[0], conv.dilation[0], conv.groups
        Ho = (x.H + 2 * p - d * (kh - 1) - 1) // s + 1
        Wo = (x.W + 2 * p - d * (kw - 1) - 1) // s + 1
        if x.buf == -1:
            kind = STEM
        elif g == cout and cin_g == 1 and x.C == cout:
            kind = DW
        elif kh == 1 and g == 1:
            kind = PW
            assert p == 0
        elif kh == 3 and g == 1 and p == 1 and d == 1:
            kind = KXK
        else:
            raise _lib.LhnError(f"unsupported convolution {tuple(conv.weight.shape)} groups={g}")
        cpad = cout
        if kind == PW:
            assert cin_g <= x.C < cin_g + 4, (cin_g, x.C)
            if not nchw_out:
                cpad = (cout + 3) // 4 * 4          # (a BatchNorm behind a padded output owns the first `cout` columns)
        elif kind == KXK:
            assert cin_g == x.C, (cin_g, x.C)
        xs = self.lazy_sources(x)
        if xs is not None:
            ok = (kind == DW and len(xs) <= 2 and kh == 3 and s == 1 and p == d and d in (1, 2) and x.C % 32 == 0 and x.W >= (8 if d == 1 else 16)
                  and conv.weight is not None) or \
                 (kind == PW and s == 1 and not nchw_out and x.C == cout and x.C in self.LAZY_PW and cin_g == x.C)
            if not ok:
                self.real(x)
                xs = None
        if nchw_out:
            assert kind == PW and bn is None and out is None
            out = TRef(-2, 0, cout, Ho, Wo)
            self.nchw_out_C = cout
            self.nchw_stacks = 1 if stack is None else int(stack[1])
        elif out is None:
            out = self.new(Ho, Wo, cpad)
        assert (out.H, out.W, out.C) == (Ho, Wo, cpad), (out, Ho, Wo, cpad)
        if out.buf >= 0:
            self.real(out)
        rec = dict(op=kind, x=x, out=out, conv=conv, bn=bn, slope=float(slope), k=kh, stride=s, pad=p, dil=d,
                   nchw=nchw_out, stack=(0, 1) if stack is None else (int(stack[0]), int(stack[1])),
                   wrc=(cout if cpad != cout else 0, cin_g if cin_g != x.C else 0), xs=xs, bn_repeat=int(bn_repeat))
        if kind == KXK:
            rec["wt"] = self._ws("misc", 9 * cout * cin_g * 4)      # tap-major weight scratch (lhn_conv_kxk_*: wt_scratch)
        if bn is not None:
            self._bn_ws(rec, max(cout, cpad), out)        # statistics are laid out for the (padded) output view
        self.recs.append(rec)
        if bn is None and not nchw_out:
            # BN-free conv (deployed RepConv/RepBlock, repblocks.py:41-43,118-119): bias and activation stay pending
            # in the output's table.  The 1x1 kernel already adds its bias while storing.
            tb = conv.bias if kind != PW else None
            if tb is not None or float(slope) != 1.0:
                if self.with_backward:
                    raise _lib.LhnError("BN-free convolutions with a pending bias/activation are inference-only (deploy form)")
                self.recs.append(dict(op=TABLE_FILL, out=out, bias=tb, slope=float(slope)))
        return out

    def bn_only(self, x, bn, slope=1.0):
        """BatchNorm applied straight to a tensor (RepBlock.rbr_identity, repblocks.py:113-114): lowered as an
        identity depthwise 1x1 (weights = NULL = ones), which copies the consumed value, takes the batch
        statistics in its epilogue and leaves the normalisation pending like any other conv+BN."""
        x = self.real(self.single(x))
        out = self.new(x.H, x.W, x.C)
        rec = dict(op=DW, x=x, out=out, conv=_IDENT, bn=bn, slope=float(slope), k=1, stride=1, pad=0, dil=1, nchw=False)
        self._bn_ws(rec, x.C, out)
        self.recs.append(rec)
        return out

    # Residual sums whose readers can add the operands while loading them (the 3x3 depthwise LDS kernel: 2 operands, the
    # square 64/128-channel 1x1: 3) are "lazy": the combine is recorded but not launched in forward; the backward pass
    # materialises it once (weight gradients need the value) and distributes its gradient like any other combine.
    LAZY_PW = (64, 128)

    def lazy_sources(self, x):
        """[(TRef, coef)] behind a lazy view x (same channel slice of every operand), or None."""
        if isinstance(x, TCat) or x.buf < 0:
            return None
        rec = self.bufs[x.buf].lazy
        if rec is None:
            return None
        return [(TRef(t.buf, t.coff + x.coff, x.C, t.H, t.W), c) for t, c in rec["flat"]]

    def real(self, x):
        """x as something every kernel can read: a lazy sum is materialised where it was recorded."""
        for p in _parts(x):
            if p.buf >= 0 and self.bufs[p.buf].lazy is not None:
                self.bufs[p.buf].lazy["lazy"] = False
                self.bufs[p.buf].lazy = None
        return x

    def ew(self, srcs, out_slope=1.0, out=None, lazy=False, mode=0, coefs=None):
        """out = act(sum of sources); smaller sources are nearest-upsampled.  Plain output.
        lazy=True (plain same-size sum into a fresh buffer): see lazy_sources().
        mode EW_MUL: product instead of sum (exactly two single-buffer sources); EW_BILINEAR: smaller sources are resampled
        bilinearly with align_corners=True.  coefs: one factor per source."""
        assert 1 <= len(srcs) <= 3
        if mode or coefs is not None:
            srcs = [self.real(self.single(t)) for t in srcs]
            assert not (mode & EW_MUL) or len(srcs) == 2
            H, W = max(t.H for t in srcs), max(t.W for t in srcs)
            if out is None:
                out = self.new(H, W, srcs[0].C)
            assert not isinstance(out, TCat) and all(t.C == out.C for t in srcs)
            self.recs.append(dict(op=EW, srcs=list(srcs), out=self.real(out), slope=float(out_slope), mode=int(mode),
                                  coefs=None if coefs is None else [float(c) for c in coefs]))
            return out
        if lazy and out is None and out_slope == 1.0 and not any(isinstance(t, TCat) for t in srcs) and \
                all((t.H, t.W, t.C) == (srcs[0].H, srcs[0].W, srcs[0].C) and t.buf >= 0 for t in srcs):
            flat = []
            for t in srcs:
                inner = self.lazy_sources(t)
                for u, c in (inner if inner is not None else [(t, 1.0)]):
                    for j, (v, cv) in enumerate(flat):
                        if (v.buf, v.coff, v.C) == (u.buf, u.coff, u.C):
                            flat[j] = (v, cv + c)
                            break
                    else:
                        flat.append((u, c))
            if len(flat) <= 3:
                out = self.new(srcs[0].H, srcs[0].W, srcs[0].C)
                rec = dict(op=EW, srcs=list(srcs), out=out, slope=1.0, lazy=True, flat=flat)
                self.bufs[out.buf].lazy = rec
                self.recs.append(rec)
                return out
        srcs = [self.real(t) for t in srcs]
        if out is not None:
            self.real(out)
        if out_slope == SLOPE_SILU and len(srcs) > 1:
            # the SiLU backward recomputes the pre-activation from its (single, same-size) source: sum first
            return self.ew([self.ew(srcs, 1.0)], SLOPE_SILU, out)
        H, W = max(s.H for s in srcs), max(s.W for s in srcs)
        if out is None:
            out = self.new(H, W, srcs[0].C)
        assert all(s.C == out.C for s in srcs)
        if any(isinstance(t, TCat) for t in list(srcs) + [out]):
            for lo, hi in self._segments(list(srcs) + [out]):      # one launch per run of channels that is one part everywhere
                self.ew([self.slice(t, lo, hi - lo) for t in srcs], out_slope, self.slice(out, lo, hi - lo))
            return out
        self.recs.append(dict(op=EW, srcs=list(srcs), out=out, slope=float(out_slope)))
        return out

    def maxpool(self, x, out=None):
        x = self.real(x)
        Ho, Wo = (x.H + 1) // 2, (x.W + 1) // 2
        if out is None:
            out = self.new(Ho, Wo, x.C)
        if isinstance(x, TCat) or isinstance(out, TCat):
            for lo, hi in self._segments([x, out]):
                self.maxpool(self.slice(x, lo, hi - lo), self.slice(out, lo, hi - lo))
            return out
        self.recs.append(dict(op=MAXPOOL, x=x, out=out))
        return out

    def avgpool(self, x, OH, OW, out=None):
        """adaptive_avg_pool2d of the consumed value -> a plain [N,OH,OW,C] buffer (one per part of a multi-part x), or into the
        channel slice `out` of an existing one (the pooled branches of CrossResolutionWeighting land side by side)."""
        x = self.real(x)
        if isinstance(x, TCat):
            assert out is None
            return TCat([self.avgpool(p, OH, OW) for p in x.parts])
        if out is None:
            out = self.new(OH, OW, x.C)
        assert (out.H, out.W, out.C) == (OH, OW, x.C)
        self.recs.append(dict(op=AVGPOOL, x=x, out=out, OH=OH, OW=OW, ca=False))
        return out

    def shuffle2(self, a, b):
        """channel_shuffle(torch.cat([a, b], 1), 2) (lite_hrnet.py:29-52): a new plain buffer with a / b interleaved."""
        a, b = self.real(self.single(a)), self.real(self.single(b))
        assert (a.H, a.W, a.C) == (b.H, b.W, b.C) and a.C % 2 == 0 and a.coff % 2 == 0 and b.coff % 2 == 0
        out = self.new(a.H, a.W, 2 * a.C)
        self.recs.append(dict(op=SHUFFLE, a=a, b=b, out=out))
        return out

    def _dpool_segments(self, y, what):
        """The backward of a 3x3-pooled attention stores its pooled gradient per segment (lhn_common.h: lhn_dpool_store), and a
        1-pixel axis lies in all three bins but in one segment only: two thirds of that gradient would be lost."""
        if self.with_backward and min(y.H, y.W) < 2:
            raise _lib.LhnError(f"{what} on a {y.H} x {y.W} map: the segment layout of the pooled gradient needs H, W >= 2 "
                                "(forward-only plans take any map)")

    def channel_attention(self, y, ca):
        """common.py:40-66 on the WHOLE buffer behind `y`: sets the buffer's gate.  Returns y."""
        b = self.bufs[y.buf]
        assert y.coff == 0 and y.C == b.C, "channel attention gates a whole buffer"
        assert not b.gate, "buffer is already gated"
        self._dpool_segments(y, "channel attention")
        Cc = y.C
        pooled = self._ws("misc", self.N * 9 * Cc * 4)
        save = self._ws("misc", (6 * self.N * Cc + 2 * Cc) * 4)          # forward rows + backward scratch (lhn_ca_mlp_bwd)
        mask = self._ws("mask", self.N * Cc * 4) if self.p_drop > 0 else None
        rec = dict(op=CA_MLP, y=y, ca=ca, pooled=pooled, save=save, mask=mask, gsum=self._ws("misc", 2 * Cc * 8))
        # gated RepBasicUnit: the copy of the pass-through half into this buffer rides in the attention's pooling launch
        # (lhn_avgpool_fwd4: copy_src); the record stays for the backward pass.  LHN_COPY_POOL=0: separate copy.
        copies = [q for q in self.recs if q["op"] == EW and not q.get("lazy") and "flat" not in q and not q.get("mode") and
                  q.get("coefs") is None and not isinstance(q["out"], TCat) and q["out"].buf == y.buf]
        writers = [q for q in self.recs if q["op"] in (STEM, PW, DW, KXK, MAXPOOL, AVGPOOL, SHUFFLE) and
                   q.get("out") is not None and not isinstance(q["out"], TCat) and q["out"].buf == y.buf]
        if _switch("LHN_COPY_POOL") and len(copies) == 1 and not hasattr(ca, "rbr_reparam"):
            q = copies[0]
            src = q["srcs"][0] if len(q["srcs"]) == 1 else None
            if src is not None and not isinstance(src, TCat) and src.buf >= 0 and src.buf != y.buf and q["slope"] == 1.0 and \
                    q["out"].coff == 0 and 0 < q["out"].C < Cc and (src.H, src.W) == (y.H, y.W) and \
                    all(w["out"].coff >= q["out"].C for w in writers) and self.bufs[src.buf].lazy is None:
                q["fwd_fused"] = True
                rec["copy"] = q
        if self.with_backward:
            rec["gsum_b"] = self._ws("misc", 2 * Cc * 8)
            rec["dgate"] = self._ws("zb", 3 * self.N * Cc * 4)         # dgate | T0, T1 of the gate-gradient pass (bnslices); zeroed with the arena
            b.dpool = True
            # BatchNorm-backward sums of the convolutions that wrote this buffer: assembled by the attention's backward from the
            # gate-gradient pass and the forward pooling pass (include/lhn.h: lhn_bn_slices) -- their lhn_bn_bwd_reduce passes
            # over the feature map and its gradient disappear.  LHN_GATE_BN_SUMS=0: separate passes.
            prods = [q for q in self.recs if q["op"] in (STEM, PW, DW, KXK) and q["bn"] is not None and
                     not isinstance(q["out"], TCat) and q["out"].buf == y.buf]
            if _switch("LHN_GATE_BN_SUMS") and 1 <= len(prods) <= 2 and not hasattr(ca, "rbr_reparam") and \
                    all(not q.get("wrc", (0, 0))[0] and q.get("bn_repeat", 1) == 1 for q in prods):
                rec["bnslices"] = prods
                rec["pstat"] = self._ws("misc", self.N * 9 * 2 * Cc * 4)
                for q in prods:
                    q["sums_by_ca"] = True
        self.recs.append(rec)
        b.gate = True
        return y

    def me_attention(self, y, att):
        """`mynet` attention (pose_hg_ms_att.py:165-174) on the WHOLE plain buffer behind `y`; `att` is the reference's
        nn.Sequential (1 = BatchNorm2d, 3 = depthwise 3x3 conv, 6 = Linear).  Sets the buffer's gate, returns y."""
        b = self.bufs[y.buf]
        assert y.coff == 0 and y.C == b.C and not b.gate, "attention gates a whole, ungated buffer"
        self._dpool_segments(y, "`mynet` attention")
        Cc = y.C
        rec = dict(op=ATT_MLP, y=y, att=att, pooled=self._ws("misc", self.N * 9 * Cc * 4),
                   save=self._ws("misc", (3 * self.N * Cc + 2 * Cc) * 4),
                   mask=self._ws("mask", self.N * Cc * 4) if self.p_drop > 0 else None, gsum=self._ws("misc", 2 * Cc * 8))
        if self.with_backward:
            rec["gsum_b"] = self._ws("misc", 2 * Cc * 8)
            rec["dgate"] = self._ws("zb", self.N * Cc * 4)
            b.dpool = True
        self.recs.append(rec)
        b.gate = True
        return y

    def se_attention(self, y, se, convs=None, mode=0, global_pool=False):
        """SEBlock (common.py:23-37) on the WHOLE buffer behind `y` (square maps: avg_pool2d(kernel=W) is global).
        convs = (down, up) Conv2d modules when they are not `se.down` / `se.up` -- or nn.Linear ones ([J, C] / [C, J], the
        same memory), with or without biases; mode 1 = SpatialWeighting of lite_hrnet.py:55-74 (global average pool,
        sigmoid(relu(.)) after both convolutions); global_pool: mode 0 behind nn.AdaptiveAvgPool2d(1), any map shape."""
        b = self.bufs[y.buf]
        assert y.coff == 0 and y.C == b.C and not b.gate, "attention gates a whole, ungated buffer"
        if y.H != y.W and mode == 0 and not global_pool:
            raise _lib.LhnError("SEBlock pools with kernel_size = width: only square maps are built")
        down, up = convs if convs is not None else (se.down, se.up)
        Cc, J = y.C, down.weight.shape[0]
        rec = dict(op=SE_MLP, y=y, se=se, down=down, up=up, mode=int(mode), J=J, pooled=self._ws("misc", self.N * Cc * 4),
                   save=self._ws("misc", self.N * (J + Cc) * 4))
        if self.with_backward:
            rec["dgate"] = self._ws("zb", self.N * Cc * 4)
            b.dpool = True
        self.recs.append(rec)
        b.gate = True
        return y

    def cbam_attention(self, x, mod):
        """CBAM (attention.py:269-294) of the plain tensor x; `mod` holds pre (biased 3x3 + BN + ReLU + biased 3x3 + BN), residual_conv
        (a biased 1x1), ca.sharedMLP (two bias-free 1x1 convolutions) and sa.conv (7x7, 2 -> 1).  pre and residual_conv are ordinary
        convolution records; one CBAM record reads p = pre's output (left UNGATED: its value is raw + table) and r, and writes the
        block's output into a new plain buffer.  Its backward hands the convolutions' backward d(loss)/d(value) of p and of r."""
        x = self.real(self.single(x))
        pre, Cc = mod.pre, mod.pre[3].weight.shape[0]
        if Cc % 16 or Cc > 256:
            raise _lib.LhnError(f"CBAM over {Cc} channels: the kernels take multiples of 16 up to 256 (the MLP has C / 16 hidden neurons)")
        t = self.conv(x, pre[0], pre[1], slope=0.0)
        p = self.conv(t, pre[3], pre[4])
        r = self.conv(x, mod.residual_conv, None)
        out = self.new(p.H, p.W, Cc)
        sv, sc = _lib.cbam_layout(self.N, p.H, p.W, Cc)
        rec = dict(op=CBAM, p=p, r=r, out=out, mod=mod, save=self._ws("misc", 4 * sv[-1]))
        if self.with_backward:
            rec["scratch"] = self._ws("misc", 4 * sc[-1])
        self.recs.append(rec)
        return out

    def set_output(self, y):
        """Generic (block-level) output: materialise the consumed value into a plain buffer."""
        self.out_ref = self.ew([y])
        return self.out_ref

    # ------------------------------------------------------------------ lowering
    def _layout(self):
        N = self.N
        base = 0
        self.arena_base = {}
        for name in ("zf", "zb", "mask", "misc"):
            self.arena_base[name] = base
            base += _al(self.ar[name].size)
        self.table_base = base
        for b in self.bufs:
            b.off["table"] = base
            base += _al(3 * b.C * 4)
        self.table_end = base
        for b in self.bufs:
            if b.gate:
                b.off["gate"] = base
                base += _al(N * b.C * 4)
            if self.with_backward and b.coef:
                b.off["coef"] = base
                base += _al(3 * b.C * 4)
            if self.with_backward and b.dpool:
                b.off["dpool"] = base
                base += _al(N * 25 * b.C * 4)      # LHN_DPOOL_SLOTS: 5 x 5 bin-overlap segments
        for b in self.bufs:
            if b.fused:                                   # lives in LDS only
                b.off["data"] = -1
                continue
            b.off["data"] = base
            if b.lazy is None or self.with_backward:      # a lazy sum is only ever written by the backward pass
                base += _al(N * b.H * b.W * b.C * 4)
        self.act_bytes = base
        if self.with_backward:
            for b in self.bufs:
                b.off["grad"] = base
                base += _al(N * b.H * b.W * b.C * 4)
        self.total_bytes = base

    def _abs(self, ref):
        return -1 if ref is None else self.arena_base[ref[0]] + ref[1]

    @staticmethod
    def _mk(kind, ins=(), out=None, p=(), ws=(), i=(), f=()):
        o = Op()
        o.kind = kind
        for k in range(3):
            o.in_buf[k] = -1
        for k, t in enumerate(ins):
            o.in_buf[k], o.in_coff[k], o.in_C[k] = t.buf, t.coff, t.C
        if out is not None:
            o.out_buf, o.out_coff, o.out_C = out.buf, out.coff, out.C
        else:
            o.out_buf = -1
        for slot, vals, fill in ((o.p, p, -1), (o.ws, ws, -1), (o.i, i, 0), (o.f, f, 0.0)):
            for k in range(len(slot)):
                slot[k] = vals[k] if k < len(vals) else fill
        return o

    def _xs(self, r):
        """(input views, number of sources, coefficient slots f[4..6]) of a convolution record: the operands of a lazy sum
        when the input still is one, else the input itself."""
        x = r["x"]
        if r.get("xs") is not None and x.buf >= 0 and self.bufs[x.buf].lazy is not None:
            views = [t for t, _ in r["xs"]]
            coefs = [c for _, c in r["xs"]]
            return views, len(views), coefs + [0.0] * (3 - len(coefs))
        return [x], 1, [1.0, 0.0, 0.0]

    def _grad_mode(self, written, t):
        """1 = store, 2 = accumulate for a write of d(value) into view t; updates the tracker."""
        ranges = written.setdefault(t.buf, [])
        lo, hi = t.coff, t.coff + t.C
        overlap = [r for r in ranges if r[0] < hi and lo < r[1]]
        if not overlap:
            ranges.append((lo, hi))
            return 1
        covered = sorted(overlap)
        cur = lo
        for a, b in covered:
            if a > cur:
                break
            cur = max(cur, b)
        if cur >= hi:
            return 2
        # partial overlap: fall back to a zeroed gradient buffer with accumulate-only writes
        self._needs_zero_grad.add(t.buf)
        ranges.append((lo, hi))
        return 2

    def _covered(self, written, t):
        """The backward op of t's producer is about to READ d(t): channels nobody wrote (an output only partly consumed) must
        read as zero -> the gradient buffer is zero-filled at the start of the backward and every write accumulates."""
        if t is None or isinstance(t, TCat) or t.buf < 0:
            return
        buf = t.buf
        while buf in self._alias_of:            # an aliased gradient buffer is written through the combine it aliases
            buf = self._alias_of[buf]
        if buf != t.buf:
            return
        cur, hi = t.coff, t.coff + t.C
        for a, b in sorted(written.get(t.buf, [])):
            if a > cur:
                break
            cur = max(cur, b)
        if cur < hi:
            self._needs_zero_grad.add(t.buf)
            written.setdefault(t.buf, []).append((t.coff, hi))

    # ------------------------------------------------------------------ inference rewrites: what the matchers and passes share
    def _uses(self):
        """buffer -> [(record, key)] for every view in every record, in record order (the matchers take the first candidate).  Every
        pass calls it on entry and nothing caches it: a pass sees the records the previous one left."""
        uses = {}
        for r in self.recs:
            for key, v in r.items():
                for t in _refs_in(v):
                    uses.setdefault(t.buf, []).append((r, key))
        return uses

    def _whole_fresh(self, t, C):
        """True when view t is the whole of a C-channel buffer that is ungated, not lazy, not fused and neither the plan's input nor its output."""
        if isinstance(t, TCat) or t.buf < 0:
            return False
        tb = self.bufs[t.buf]
        if t.coff != 0 or t.C != C or tb.C != C or tb.gate or tb.lazy is not None or tb.fused:
            return False
        return not any(v is not None and v.buf == t.buf for v in (self.in_ref, self.out_ref))

    def _sole_reader(self, t, writer, uses, kind):
        """The only record that reads the whole fresh buffer behind view t (written by `writer`), if it is of `kind`; else None.  What
        fills the buffer's table (FINALIZE / TABLE_FILL) is not a reader."""
        if not self._whole_fresh(t, t.C):
            return None
        q = None
        for u, key in uses.get(t.buf, ()):
            if (u is writer or u["op"] in (FINALIZE, TABLE_FILL)) and key == "out":
                continue
            if u["op"] == kind and key in ("x", "srcs") and q is None:
                q = u
                continue
            return None
        return q

    def _plain_conv(self, r, kind, biased_bn=False):
        """A stride-1 convolution record of `kind` with one plain source and nothing special about its weights or BatchNorm (biased_bn:
        a bias in front of a BatchNorm is fine -- the caller's kernel adds it ahead of the table)."""
        if r is None or r["op"] != kind or r["stride"] != 1 or r["nchw"] or r["wrc"] != (0, 0) or r["bn_repeat"] != 1 or self._xs(r)[1] != 1:
            return False
        if r["x"].buf < 0 or isinstance(r["x"], TCat):
            return False
        return biased_bn or not _biased_bn(r)

    def _plain_dw3(self, q, dils, max_srcs=1):
        """A 3x3 depthwise convolution record with weights: stride 1, padding == dilation in `dils`, at most max_srcs summed sources and
        no bias in front of a BatchNorm."""
        if q is None or q["op"] != DW or (q["k"], q["stride"]) != (3, 1) or q["pad"] != q["dil"] or q["dil"] not in dils:
            return False
        if q["conv"].weight is None or q.get("bn_repeat", 1) != 1 or self._xs(q)[1] > max_srcs or q["x"].buf < 0:
            return False
        return not _biased_bn(q)

    @staticmethod
    def _tables(q, fill=False, bias=False):
        """The records that fill the table of convolution record q's output without q: FINALIZE when q has a BatchNorm; else, with `fill`,
        a TABLE_FILL for its pending bias / activation.  fuse_pw_dw and fuse_msrb_round drop the original TABLE_FILL and emit this one
        ahead of their launch; the other passes leave the original where it stands and ask for none.  `bias` (fuse_ccw): the FINALIZE
        folds a bias in front of the BatchNorm into the shift, as the unfused convolution's own finalize does, and covers the
        BatchNorm's channels only (a 7 / 17 / 37-wide one sits in a view padded to a multiple of 4)."""
        if q["bn"] is not None and bias:
            t = q["out"]
            return [dict(op=FINALIZE, out=TRef(t.buf, t.coff, q["bn"].num_features, t.H, t.W), bn=q["bn"], slope=q["slope"], bias=q["conv"].bias)]
        if q["bn"] is not None:
            return [dict(op=FINALIZE, out=q["out"], bn=q["bn"], slope=q["slope"])]
        if fill and (q["conv"].bias is not None or q["slope"] != 1.0):
            return [dict(op=TABLE_FILL, out=q["out"], bias=q["conv"].bias, slope=q["slope"])]
        return []

    def _splice(self, at, drop):
        """Rebuild the record list: a record whose id is in `at` is replaced by the list there, one whose id is in `drop` disappears,
        the rest stay.  Returns the number of replacements."""
        recs = []
        for r in self.recs:
            recs += at.get(id(r), [] if id(r) in drop else [r])
        self.recs = recs
        return len(at)

    # Channel counts lhn_conv_pw_dw3_fwd is built for (csrc/k_conv_pwdw.hip: pw_dw3_supported); any map size.
    FUSE_PW_DW_CHANNELS = (64,)

    def _fusable_pw_dw(self, r, uses):
        """The depthwise record that can share a launch with the 1x1 record r, or None.  The pair: a stride-1 1x1 of one plain
        source into a whole fresh buffer whose ONLY reader is a 3x3 depthwise convolution (stride 1, dilation 1, padding 1,
        one source) over all of it, with channel counts the entry point accepts."""
        if not self._plain_conv(r, PW):
            return None
        x, t = r["x"], r["out"]
        if x.C not in self.FUSE_PW_DW_CHANNELS or not self._whole_fresh(t, x.C):
            return None
        q = None
        for u, key in uses.get(t.buf, ()):
            if u is r and key == "out":
                continue
            if u["op"] == TABLE_FILL and key == "out":       # deployed form: the 1x1's pending activation
                continue
            if u["op"] == DW and key == "x" and q is None:
                q = u
                continue
            return None
        if not self._plain_dw3(q, (1,)):
            return None
        qx, y = q["x"], q["out"]
        if (qx.coff, qx.C) != (0, t.C) or y.C != t.C or y.buf == t.buf or _overlaps(x, y):
            return None
        return q

    def fuse_pw_dw(self):
        """Inference plans with the switch on (infer_fuse): RepBasicUnit's right branch, RepConv 1x1 then RepConv depthwise 3x3
        (litehourglass.py:52-78), becomes ONE launch.  Without train-mode BatchNorm the transform between the two convolutions
        is known before the launch: it is written into the intermediate buffer's table by what fills it in the unfused plan
        (eval: FINALIZE from the running statistics; deployed: TABLE_FILL with the 1x1's bias, which the unfused 1x1 adds while
        storing), the fused kernel reads it as t_table, and the intermediate buffer gets no data.  Both table launches sit
        under LHN_RUN_TABLES_CURRENT like every other.  The launch stands where the depthwise convolution stood.  Plans with a
        backward are never rewritten."""
        if self.with_backward or not self.infer_fuse:
            return 0
        uses = self._uses()
        at, drop = {}, set()
        for r in self.recs:
            q = self._fusable_pw_dw(r, uses)
            if q is None:
                continue
            t = r["out"]
            at[id(q)] = self._tables(r, fill=True) + [dict(op=PWDW, x=r["x"], mid=t, out=q["out"], conv=r["conv"], conv2=q["conv"])] + \
                self._tables(q)
            drop |= {id(r)} | {id(u) for u, key in uses[t.buf] if u["op"] == TABLE_FILL and key == "out"}
            self.bufs[t.buf].fused = True
        n = self._splice(at, drop)
        self.n_fused += n
        return n

    # Channel counts and dilations lhn_conv_dw3_pw_fwd is built for (csrc/k_conv_dwpw.hip: dw3_pw_supported); any map size.
    FUSE_DW_PW_CHANNELS = (32, 64)
    FUSE_DW_PW_DILATIONS = (1, 2)

    def _fusable_dw_pw(self, q, uses):
        """The 1x1 record that can share a launch with the depthwise record q, or None.  The pair: a 3x3 depthwise convolution
        (stride 1, padding == dilation, one plain source) into a whole fresh buffer whose ONLY reader is a stride-1 1x1 of one
        source over all of it, with channel counts the entry point accepts."""
        if not self._plain_dw3(q, self.FUSE_DW_PW_DILATIONS):
            return None
        x, t = q["x"], q["out"]
        if x.C not in self.FUSE_DW_PW_CHANNELS or not self._whole_fresh(t, x.C):
            return None
        r = None
        for u, key in uses.get(t.buf, ()):
            if u is q and key == "out":
                continue
            if u["op"] == TABLE_FILL and key == "out":       # deployed form: the depthwise convolution's pending bias / activation
                continue
            if u["op"] == PW and key == "x" and r is None:
                r = u
                continue
            return None
        if not self._plain_conv(r, PW):
            return None
        rx, y = r["x"], r["out"]
        if (rx.coff, rx.C) != (0, t.C) or y.C not in self.FUSE_DW_PW_CHANNELS or y.buf == t.buf or _overlaps(x, y):
            return None
        return r

    def fuse_dw_pw(self):
        """Inference plans with the switch on (infer_fuse_dwpw): DWConv, RepConv depthwise 3x3 (dilation 1 or 2) then RepConv 1x1
        (liteHandNet.py:8-21), becomes ONE launch.  As in fuse_pw_dw the transform between the two convolutions is written into the
        intermediate buffer's table by what fills it in the unfused plan (eval: FINALIZE from the running statistics; deployed: the
        TABLE_FILL with the depthwise convolution's bias, which stays where it is), the fused kernel reads it as t_table, and the
        intermediate buffer gets no data.  The launch stands where the 1x1 stood.  Plans with a backward are never rewritten."""
        if self.with_backward or not self.infer_fuse_dwpw:
            return 0
        uses = self._uses()
        at, drop = {}, set()
        for q in self.recs:
            r = self._fusable_dw_pw(q, uses)
            if r is None:
                continue
            t = q["out"]
            fused = dict(op=DWPW, x=q["x"], mid=t, out=r["out"], conv=q["conv"], conv2=r["conv"], dil=q["dil"],
                         bias=None if r["bn"] is not None else r["conv"].bias)
            at[id(r)] = self._tables(q) + [fused] + self._tables(r)
            drop.add(id(q))
            self.bufs[t.buf].fused = True
        n = self._splice(at, drop)
        self.n_fused_dwpw += n
        return n

    # Channels per half lhn_msrb_round_fwd is built for (csrc/k_msrb.hip: msrb_half_ok); any map size.
    FUSE_MSRB_HALF = (32, 64, 128)

    def _msrb_branch(self, q, dil):
        """True when the record q can be one branch of a fused MSRB round: a 3x3 depthwise convolution, stride 1, dilation ==
        padding == dil, of at most two summed sources, over a channel count the entry point accepts."""
        if not self._plain_dw3(q, (dil,), max_srcs=2):
            return False
        x, y = q["x"], q["out"]
        return y.buf >= 0 and x.C == y.C and y.C in self.FUSE_MSRB_HALF

    def fuse_msrb_round(self):
        """Inference plans with the switch on (infer_fuse_msrb): one round of an MSRB (litehourglass.py:43-50) -- the depthwise 3x3
        at dilation 1 into the lower half of a buffer, the one at dilation 2 into its upper half and, when a ChannelAttension /
        SEBlock gates that buffer, the average pool its MLP reads -- becomes ONE record (lhn_msrb_round_fwd).  The pooling needs
        the consumed value of what the launch has just computed, so the pending tables of both halves are emitted ahead of it by
        what fills them in the unfused plan (eval: FINALIZE from the running statistics; deployed: TABLE_FILL with the bias), under
        LHN_RUN_TABLES_CURRENT like every other table launch.  The launch stands where the second convolution stood.  Plans with a
        backward are never rewritten."""
        if self.with_backward or not self.infer_fuse_msrb:
            return 0
        uses = self._uses()
        order = {id(r): j for j, r in enumerate(self.recs)}
        at, drop = {}, set()
        for b, rec in enumerate(self.bufs):
            if rec.lazy is not None or rec.fused or any(v is not None and v.buf == b for v in (self.in_ref, self.out_ref)):
                continue
            wr = [u for u, key in uses.get(b, ()) if key == "out"]
            dws = [u for u in wr if u["op"] == DW]
            fills = [u for u in wr if u["op"] == TABLE_FILL]
            if len(dws) != 2 or len(dws) + len(fills) != len(wr):
                continue
            q1, q2 = dws if dws[0]["dil"] == 1 else dws[::-1]
            h = q1["out"].C
            if not (self._msrb_branch(q1, 1) and self._msrb_branch(q2, 2)) or q2["out"].C != h or rec.C != 2 * h or \
                    (q1["out"].coff, q2["out"].coff) != (0, h):
                continue
            (v1, n1, c1), (v2, n2, c2) = self._xs(q1), self._xs(q2)
            if n1 != n2 or c1 != c2 or any(v.buf == b or v.buf < 0 for v in v1 + v2):
                continue
            lo, hi = sorted((order[id(q1)], order[id(q2)]))
            if any(not (u["op"] == TABLE_FILL and u["out"].buf == b) for u in self.recs[lo + 1:hi]):
                continue
            gates = [u for u, key in uses.get(b, ()) if key == "y" and u["op"] in (CA_MLP, SE_MLP, ATT_MLP)]
            att = gates[0] if len(gates) == 1 and gates[0]["op"] in (CA_MLP, SE_MLP) and not gates[0].get("copy") and \
                not gates[0].get("bnslices") and order[id(gates[0])] > hi else None
            out = TRef(b, 0, 2 * h, rec.H, rec.W)
            fused = dict(op=MSRB, x0=v1[0], x1=v2[0], e0=v1[1] if n1 > 1 else None, e1=v2[1] if n1 > 1 else None, coefs=(c1[0], c1[1]),
                         out=out, conv=q1["conv"], conv2=q2["conv"], pooled=None, scratch=None, OH=0)
            if att is not None:
                nbytes = _lib.lib().lhn_msrb_round_scratch_bytes(self.N, rec.H, rec.W, 2 * h)
                if nbytes <= 0:
                    continue
                att["pool_fused"] = True        # _fwd_ca / _fwd_se: no AVGPOOL launch, the fused record fills `pooled`
                fused.update(pooled=att["pooled"], scratch=self._ws("misc", nbytes), OH=3 if att["op"] == CA_MLP else 1)
            at[id(self.recs[hi])] = self._tables(q1, fill=True) + self._tables(q2, fill=True) + [fused]
            drop |= {id(q1), id(q2)} | {id(u) for u in fills}
        n = self._splice(at, drop)
        self.n_fused_msrb += n
        return n

    # Channel pairs (C, Cm) lhn_bottleneck_fwd is built for (csrc/k_bottleneck.hip: bottleneck_supported); any map size.
    FUSE_BNECK_CHANNELS = ((128, 32), (128, 64), (256, 64), (256, 128))

    def _fusable_bottleneck(self, r1, uses):
        """(r2, r3, ew) when the 1x1 record r1 starts a BottleNeck pattern, else None: 1x1 C -> Cm, 3x3 Cm -> Cm, 1x1 Cm -> C (slope 1),
        each into a whole fresh buffer with one reader, and a plain two-source sum of r1's input and the last output."""
        if not self._plain_conv(r1, PW):
            return None
        x, t1 = r1["x"], r1["out"]
        if (x.C, t1.C) not in self.FUSE_BNECK_CHANNELS:
            return None
        r2 = self._sole_reader(t1, r1, uses, KXK)
        if not self._plain_conv(r2, KXK) or (r2["x"].coff, r2["x"].C) != (0, t1.C) or r2["out"].C != t1.C:
            return None
        t2 = r2["out"]
        r3 = self._sole_reader(t2, r2, uses, PW)
        if not self._plain_conv(r3, PW) or (r3["x"].coff, r3["x"].C) != (0, t2.C) or r3["out"].C != x.C or r3["slope"] != 1.0:
            return None
        t3 = r3["out"]
        ew = self._sole_reader(t3, r3, uses, EW)
        if ew is None or ew.get("mode") or ew.get("coefs") is not None or ew.get("lazy") or "flat" in ew or len(ew["srcs"]) != 2:
            return None
        if not 0.0 <= ew["slope"] <= 1.0 or len({t1.buf, t2.buf, t3.buf, x.buf}) != 4:
            return None
        a, b = ew["srcs"]
        key = lambda v: None if isinstance(v, TCat) else (v.buf, v.coff, v.C, v.H, v.W)
        if {key(a), key(b)} != {key(x), key(t3)} or key(x) == key(t3):
            return None
        y = ew["out"]
        if isinstance(y, TCat) or y.buf < 0 or y.buf in (t1.buf, t2.buf, t3.buf) or (y.H, y.W, y.C) != (x.H, x.W, x.C) or _overlaps(x, y):
            return None
        return r2, r3, ew

    def fuse_bottleneck(self):
        """Inference plans with the switch on (infer_fuse_bneck): BottleNeck (liteHandNet.py:23-37) -- RepConv 1x1, RepConv 3x3, RepConv
        1x1, the residual sum and its activation -- becomes ONE record (lhn_bottleneck_fwd).  The pass matches the record pattern, not
        the module class.  As in fuse_dw_pw the three intermediate buffers keep their tables and lose their data; what fills those
        tables in the unfused plan stays ahead of the launch (eval: FINALIZE from the running statistics; deployed: the TABLE_FILL
        records, which stay where they are; b1 / b3 are the 1x1 biases the unfused kernel adds while storing).  The launch stands
        where the sum stood.  Plans with a backward are never rewritten."""
        if self.with_backward or not self.infer_fuse_bneck:
            return 0
        uses = self._uses()
        at, drop = {}, set()
        for r1 in self.recs:
            m = self._fusable_bottleneck(r1, uses)
            if m is None:
                continue
            r2, r3, ew = m
            if {id(r1), id(r2), id(r3), id(ew)} & drop:
                continue
            fused = dict(op=BNECK, x=r1["x"], mids=[r1["out"], r2["out"], r3["out"]], out=ew["out"], convs=(r1["conv"], r2["conv"], r3["conv"]),
                         b1=None if r1["bn"] is not None else r1["conv"].bias, b3=None if r3["bn"] is not None else r3["conv"].bias,
                         slope=ew["slope"], wt=r2["wt"])
            at[id(ew)] = [t for q in (r1, r2, r3) for t in self._tables(q)] + [fused]
            drop |= {id(r1), id(r2), id(r3), id(ew)}
            for q in (r1, r2, r3):
                self.bufs[q["out"].buf].fused = True
        n = self._splice(at, drop)
        self.n_fused_bneck += n
        return n

    # What lhn_stem_tail_fwd is built for (csrc/k_stem.hip: stem_tail_supported): (m, C) and the depthwise kernel sizes it absorbs; any map.
    FUSE_STEM_CHANNELS = (32, 128)
    FUSE_STEM_K = (3, 7)

    def _fusable_stem(self, mp, uses):
        """(dw or None, r1, r2, r3) when the MAXPOOL record mp is branch2 of a stem (liteHandNet.py:169-193), else None: mp pools a whole
        fresh m-channel buffer t into channels [m, 2m) of a 2m-channel buffer cat; t's only other reader is a plain 1x1 (m -> m) whose
        sole reader is a 3x3 (stride 2, pad 1) into channels [0, m) of cat; cat's sole reader is a plain 1x1 (2m -> C).  dw: t's writer
        when that is a plain depthwise K x K (K in FUSE_STEM_K, stride 1, pad K / 2) the launch can absorb."""
        m, Cout = self.FUSE_STEM_CHANNELS
        t, po = mp["x"], mp["out"]
        if not self._whole_fresh(t, m) or isinstance(po, TCat) or po.buf < 0 or (po.coff, po.C) != (m, m):
            return None
        cat = TRef(po.buf, 0, 2 * m, po.H, po.W)
        if not self._whole_fresh(cat, 2 * m) or cat.buf == t.buf:
            return None
        ok_slope = lambda q: 0.0 <= q.get("slope", 1.0) <= 1.0
        r1, writers = None, []
        for u, key in uses.get(t.buf, ()):
            if key == "out":
                writers.append(u)
            elif u is mp and key == "x":
                continue
            elif u["op"] == PW and key == "x" and r1 is None:
                r1 = u
            else:
                return None
        if not self._plain_conv(r1, PW, True) or (r1["x"].coff, r1["x"].C) != (0, m) or not ok_slope(r1) or not self._whole_fresh(r1["out"], m):
            return None
        u_ = r1["out"]
        r2 = self._sole_reader(u_, r1, uses, KXK)
        if r2 is None or (r2["k"], r2["stride"], r2["pad"], r2["dil"]) != (3, 2, 1, 1) or r2["nchw"] or r2["wrc"] != (0, 0) or \
                r2["bn_repeat"] != 1 or self._xs(r2)[1] != 1:
            return None
        v = r2["out"]
        if (r2["x"].coff, r2["x"].C) != (0, m) or isinstance(v, TCat) or (v.buf, v.coff, v.C) != (cat.buf, 0, m) or not ok_slope(r2):
            return None
        r3 = None
        for u, key in uses.get(cat.buf, ()):
            if (u is r2 or u is mp) and key == "out":
                continue
            if u["op"] in (FINALIZE, TABLE_FILL) and key == "out" and (u["out"].coff, u["out"].C) == (0, m) and ok_slope(u):
                continue
            if u["op"] == PW and key == "x" and r3 is None:
                r3 = u
                continue
            return None
        if not self._plain_conv(r3, PW) or (r3["x"].coff, r3["x"].C) != (0, 2 * m):
            return None
        y = r3["out"]
        if isinstance(y, TCat) or y.buf < 0 or y.C != Cout or len({t.buf, u_.buf, cat.buf, y.buf}) != 4:
            return None
        dw = None
        convs = [q for q in writers if q["op"] in (STEM, PW, DW, KXK)]
        if len(convs) == 1 and len(convs) + sum(q["op"] in (FINALIZE, TABLE_FILL) for q in writers) == len(writers):
            q = convs[0]
            if q["op"] == DW and q["k"] in self.FUSE_STEM_K and (q["stride"], q["dil"], q["pad"]) == (1, 1, q["k"] // 2) and \
                    q["conv"].weight is not None and q.get("bn_repeat", 1) == 1 and self._xs(q)[1] == 1 and not isinstance(q["x"], TCat) and \
                    q["x"].buf >= 0 and q["x"].C == m and q["x"].buf not in (t.buf, u_.buf, cat.buf):
                dw = q
        x = dw["x"] if dw is not None else t
        # every table the launch applies holds a leaky slope: SiLU / relu-sigmoid leave the plan as it is
        for b in {x.buf, t.buf}:
            if any(key == "out" and q["op"] in (STEM, PW, DW, KXK, FINALIZE, TABLE_FILL) and not ok_slope(q) for q, key in uses.get(b, ())):
                return None
        if _overlaps(x, y):
            return None
        return dw, r1, r2, r3

    def fuse_stem(self):
        """Inference plans with the switch on (infer_fuse_stem): everything after the stem's first convolution (Stem, liteHandNet.py:169-193;
        my_pelee_stem, models/pose_hg_ms_att.py:196-228) becomes ONE record (lhn_stem_tail_fwd).  The pass matches the record pattern of
        _fusable_stem, not the module class.  K = the absorbed depthwise convolution's kernel size (t keeps its table and loses its data),
        or 0 when t is written by something else (the eval-mode RepBlock sum) and stays.  u and the concatenation buffer become
        table-only; what fills the tables in the unfused plan stays ahead of the launch (eval: FINALIZE from the running statistics;
        deployed: the TABLE_FILL records, which stay where they are).  Biases: a 1x1 without a BatchNorm adds its bias while storing,
        so b1 / b3 ride in the launch; a bias in FRONT of a BatchNorm (mynet's branch1) is folded into the table's shift by the unfused
        convolution's own finalize, which a FINALIZE record does not do, so it rides in the launch too (bT, b1, b2).
        The launch stands where the last 1x1 stood.  Runs first in finalize().  Plans with a backward are never rewritten."""
        if self.with_backward or not self.infer_fuse_stem:
            return 0
        uses = self._uses()
        at, drop = {}, set()
        for mp in self.recs:
            if mp["op"] != MAXPOOL:
                continue
            found = self._fusable_stem(mp, uses)
            if found is None:
                continue
            dw, r1, r2, r3 = found
            absorbed = [q for q in (dw, r1, r2) if q is not None]
            if {id(q) for q in absorbed + [mp, r3]} & drop:
                continue
            fused = dict(op=STEMTAIL, x=dw["x"] if dw is not None else mp["x"], t=mp["x"], u=r1["out"],
                         cat=TRef(r2["out"].buf, 0, 2 * r2["out"].C, r2["out"].H, r2["out"].W), out=r3["out"], K=dw["k"] if dw is not None else 0,
                         dw=dw["conv"] if dw is not None else None, convs=(r1["conv"], r2["conv"], r3["conv"]),
                         bT=dw["conv"].bias if dw is not None and dw["bn"] is not None else None, b1=r1["conv"].bias,
                         b2=r2["conv"].bias if r2["bn"] is not None else None, b3=None if r3["bn"] is not None else r3["conv"].bias, wt=r2["wt"])
            at[id(r3)] = [t for q in absorbed for t in self._tables(q)] + [fused] + self._tables(r3)
            drop |= {id(q) for q in absorbed + [mp, r3]}
            for q in absorbed:
                self.bufs[q["out"].buf].fused = True       # t (when absorbed), u and -- through v -- the whole concatenation buffer
        n = self._splice(at, drop)
        self.n_fused_stem += n
        return n

    def mark_bf16x3(self):
        """Inference plans with the switch on (infer_bf16x3): every dense 3x3 record that bf16x3_eligible accepts runs on the bf16 MFMA
        with a three-term split (lhn_conv_kxk_fwd_bf16x3).  The record stays a KXK record with the same views, parameters and scratch
        (the fp32 tap-major copy and the split image are both 9 * Cout * Cin * 4 bytes); it lowers to the same op with i[1] = 1.  Runs
        after fuse_bottleneck: a BNECK record keeps its fp32 inner 3x3, this pass takes the 3x3 records that are left.  Plans with a
        backward are never marked."""
        if self.with_backward or not self.infer_bf16x3:
            return 0
        n = 0
        for r in self.recs:
            if r["op"] != KXK or isinstance(r["x"], TCat) or isinstance(r["out"], TCat) or r["x"].buf < 0 or r["out"].buf < 0:
                continue
            x, y = r["x"], r["out"]
            if r["k"] == 3 and r["pad"] == 1 and r["dil"] == 1 and bf16x3_eligible(x.C, y.C, r["stride"], _overlaps(x, y)):
                r["bf16x3"] = True
                n += 1
        self.n_bf16x3 += n
        return n

    # What the lhn_ccw_* entry points are built for (csrc/k_hrnet.hip: CCW_MAX_C, CCW_MAX_CT, CCW_MAX_MID), and the numbers of branches the
    # pass rewrites.  The entry points take 2..4; the two-branch blocks (stage 2: the largest maps, 12 launches saved per block) did not
    # pass the keep-or-drop rule on their own and are left as they are (profiles/infer_fuse_ccw.md).
    FUSE_CCW_MAX = (160, 320, 40)
    FUSE_CCW_BRANCHES = (3, 4)

    def _sole_act(self, r, uses):
        """The sigmoid(relu(.)) combine that is the only reader of the 1x1 record r's output, or None."""
        e = self._sole_reader(r["out"], r, uses, EW)
        if e is None or e.get("mode") or e.get("coefs") is not None or e.get("lazy") or "flat" in e or len(e["srcs"]) != 1:
            return None
        t, y = e["srcs"][0], e["out"]
        if e["slope"] != SLOPE_RELU_SIGMOID or isinstance(t, TCat) or (t.buf, t.coff, t.C) != (r["out"].buf, 0, r["out"].C):
            return None
        return e if self._whole_fresh(y, t.C) and (y.H, y.W) == (t.H, t.W) else None

    def _ccw_pw(self, r):
        """True when r is one of CrossResolutionWeighting's 1x1 convolutions: stride 1, one plain source, a BatchNorm (a bias in front
        of it is fine, and so is a 7 / 17 / 37-wide side padded to a multiple of 4) and no activation of its own."""
        return r is not None and r["op"] == PW and r["stride"] == 1 and not r["nchw"] and r["bn_repeat"] == 1 and self._xs(r)[1] == 1 and \
            r["bn"] is not None and r["slope"] == 1.0 and not isinstance(r["x"], TCat) and r["x"].buf >= 0

    def _fusable_ccw(self, r1, uses):
        """The records of the ConditionalChannelWeighting block (lite_hrnet.py:76-143) whose first 1x1 is r1, or None.  The pattern: B =
        2..4 adaptive average pools to one (hm, wm) that tile a whole fresh buffer; r1 (Ct -> mid, BatchNorm) over all of it, a
        sigmoid(relu(.)) combine, a second 1x1 (mid -> Ct, BatchNorm) and its combine into g; per branch a product of the pooled view
        with its slice of g, a 3x3 depthwise convolution + BatchNorm of that product into a buffer of its own, a SpatialWeighting gate
        (SE_MLP mode 1) on that buffer and a SHUFFLE of it behind a view like the pooled one -- each intermediate with that one reader.
        Maps ordered from the largest to the smallest and integer multiples of the last."""
        cmax, ctmax, midmax = self.FUSE_CCW_MAX
        if not self._ccw_pw(r1):
            return None
        P = r1["x"]
        if not self._whole_fresh(P, P.C) or P.C > ctmax:
            return None
        pools = []
        for u, key in uses.get(P.buf, ()):
            if u["op"] == AVGPOOL and key == "out" and not u["ca"] and (u["OH"], u["OW"]) == (P.H, P.W):
                pools.append(u)
            elif not (u is r1 and key == "x"):
                return None
        pools.sort(key=lambda u: u["out"].coff)
        B, off = len(pools), 0
        if B not in self.FUSE_CCW_BRANCHES:
            return None
        for u in pools:
            x = u["x"]
            if isinstance(x, TCat) or x.buf < 0 or (u["out"].coff, u["out"].C) != (off, x.C) or x.C > cmax or x.H % P.H or x.W % P.W:
                return None
            off += x.C
        if off != P.C or any(a["x"].H < b["x"].H or a["x"].W < b["x"].W for a, b in zip(pools, pools[1:])) or \
                (pools[-1]["x"].H, pools[-1]["x"].W) != (P.H, P.W):
            return None
        mid = r1["conv"].weight.shape[0]
        e1 = self._sole_act(r1, uses)
        if e1 is None or mid > midmax or r1["bn"].num_features != mid or r1["conv"].weight.shape[1] != P.C:
            return None
        r2 = self._sole_reader(e1["out"], e1, uses, PW)
        if not self._ccw_pw(r2) or tuple(r2["conv"].weight.shape[:2]) != (P.C, mid) or r2["out"].C != P.C or r2["bn"].num_features != P.C:
            return None
        e2 = self._sole_act(r2, uses)
        if e2 is None or len({P.buf, r1["out"].buf, e1["out"].buf, r2["out"].buf, e2["out"].buf}) != 5:
            return None
        g = e2["out"]
        muls = [u for u, key in uses.get(g.buf, ()) if not (u is e2 and key == "out")]
        if len(muls) != B or len({id(u) for u in muls}) != B:
            return None
        branches, off = [], 0
        for pool in pools:
            x2 = pool["x"]
            m = next((u for u in muls if u["op"] == EW and u.get("mode") == EW_MUL and len(u["srcs"]) == 2 and
                      not isinstance(u["srcs"][1], TCat) and (u["srcs"][1].buf, u["srcs"][1].coff, u["srcs"][1].C) == (g.buf, off, x2.C)), None)
            off += x2.C
            if m is None or m.get("coefs") is not None or m["slope"] != 1.0 or m["srcs"][0] != x2:
                return None
            dw = self._sole_reader(m["out"], m, uses, DW)
            if dw is None or (dw["k"], dw["stride"], dw["pad"], dw["dil"]) != (3, 1, 1, 1) or dw["conv"].weight is None or dw["bn"] is None or \
                    dw["slope"] != 1.0 or dw.get("bn_repeat", 1) != 1 or self._xs(dw)[1] != 1 or (dw["x"].coff, dw["x"].C) != (0, x2.C):
                return None
            y = dw["out"]
            if isinstance(y, TCat) or y.buf < 0 or (y.coff, y.C) != (0, x2.C) or self.bufs[y.buf].C != x2.C or \
                    any(v is not None and v.buf == y.buf for v in (self.in_ref, self.out_ref)):
                return None
            se = sh = None
            for u, key in uses.get(y.buf, ()):
                if u is dw and key == "out":
                    continue
                if u["op"] == SE_MLP and key == "y" and se is None:
                    se = u
                elif u["op"] == SHUFFLE and key == "b" and sh is None:
                    sh = u
                else:
                    return None
            if se is None or sh is None or se["mode"] != 1 or se.get("pool_fused") or not 1 <= se["J"] <= midmax:
                return None
            x1, out = sh["a"], sh["out"]
            if isinstance(x1, TCat) or x1.buf < 0 or (x1.H, x1.W, x1.C) != (x2.H, x2.W, x2.C) or sh["b"] != y or not self._whole_fresh(out, 2 * x2.C):
                return None
            if out.buf in (x1.buf, x2.buf, y.buf) or y.buf in (x1.buf, x2.buf, g.buf, P.buf):
                return None
            branches.append(dict(pool=pool, mul=m, dw=dw, se=se, sh=sh, x2=x2, x1=x1, y=y, out=out))
        return dict(r1=r1, e1=e1, r2=r2, e2=e2, mid=mid, pooled=P, g=g, branches=branches)

    def fuse_ccw(self):
        """Inference plans with the switch on (infer_fuse_ccw): a ConditionalChannelWeighting block of Lite-HRNet (lite_hrnet.py:110-143)
        -- per branch a pool into the concatenation, a product with the upsampled gate, a depthwise 3x3, SpatialWeighting's pool and MLP
        and a channel shuffle, and the two 1x1 + activation pairs they share: 16 / 22 / 28 launches over 2 / 3 / 4 branches -- becomes
        FOUR records, each one launch over all branches: CCW_POOL, CCW_GATE, CCW_DW (which also leaves the per-tile sums SpatialWeighting
        pools from) and CCW_SHUFFLE (which folds them, runs the MLP and applies the gate while shuffling).  The pass matches the record
        pattern of _fusable_ccw, not the module class.  The buffers between the steps that the launches keep in registers -- both 1x1
        outputs, the first activation and the products -- keep their tables and lose their data.  The tables the launches read (both
        1x1 BatchNorms and the depthwise ones, biases folded in) are emitted ahead of them by what fills them without the convolution
        (_tables), under LHN_RUN_TABLES_CURRENT like every other table launch.  The records stand where the last shuffle stood.  A block
        whose maps are not integer multiples of its smallest one stays as it is, and so does one whose number of branches is not in
        FUSE_CCW_BRANCHES.  Plans with a backward are never rewritten."""
        if self.with_backward or not self.infer_fuse_ccw:
            return 0
        uses = self._uses()
        order = {id(r): j for j, r in enumerate(self.recs)}
        at, drop = {}, set()
        for r1 in self.recs:
            m = self._fusable_ccw(r1, uses)
            if m is None:
                continue
            br = m["branches"]
            nbytes = _lib.lib().lhn_ccw_scratch_bytes(self.N, len(br), *((C.c_int * len(br))(*[getattr(b["x2"], k) for b in br]) for k in "HWC"))
            if nbytes <= 0:
                continue
            scratch = self._ws("misc", nbytes)
            x2, x1, ys, outs = ([b[k] for b in br] for k in ("x2", "x1", "y", "out"))
            args = dict(x2=x2, x1=x1, ys=ys, outs=outs, dws=[b["dw"]["conv"] for b in br], ses=[(b["se"]["down"], b["se"]["up"], b["se"]["J"]) for b in br])
            fused = [dict(op=CCW_POOL, out=m["pooled"], **args),
                     dict(op=CCW_GATE, x=m["pooled"], mids=[m["r1"]["out"], m["r2"]["out"]], out=m["g"], conv=m["r1"]["conv"], conv2=m["r2"]["conv"],
                          mid=m["mid"]),
                     dict(op=CCW_DW, g=m["g"], scratch=scratch, **args),
                     dict(op=CCW_SHUFFLE, scratch=scratch, **args)]
            old = [m["r1"], m["e1"], m["r2"], m["e2"]] + [b[k] for b in br for k in ("pool", "mul", "dw", "se", "sh")]
            last = max(old, key=lambda u: order[id(u)])
            at[id(last)] = [t for q in [m["r1"], m["r2"]] + [b["dw"] for b in br] for t in self._tables(q, bias=True)] + fused
            drop |= {id(u) for u in old}
            for t in [m["r1"]["out"], m["e1"]["out"], m["r2"]["out"]] + [b["mul"]["out"] for b in br]:
                self.bufs[t.buf].fused = True
        n = self._splice(at, drop)
        self.n_fused_ccw += n
        return n

    # ------------------------------------------------------------------ finalize: the passes in the order they run
    def finalize(self):
        """Lower the records to what lhn_plan_create takes: (Buf array, forward Op array, backward Op array or None, n_fwd, n_bwd)."""
        for _, _, method, _, _ in INFER_SWITCHES:
            getattr(self, method)()
        self._layout()
        self._plan_sum_out()
        fwd = self._lower_forward()
        bwd = self._lower_backward() if self.with_backward else []
        self.sync_points = self._sync_points(fwd, bwd)
        return self._c_arrays(fwd, bwd)

    def _plan_sum_out(self):
        """Plans with a backward: a convolution that sums a lazy residual on load also WRITES the sum (lhn_pw_opts.sum_out) when
        the readers' channel slices cover the buffer -- the weight gradients of the backward then find it in memory and the
        re-materialising combine (which re-reads every operand) is not needed.  LHN_SUM_OUT=0: re-materialise."""
        self.sum_out = {}               # id(conv record) -> (byte offset of the sum's buffer, pixel stride * 65536 + channel)
        self._sum_written = set()       # lazy buffers complete after the forward
        if not (self.with_backward and _switch("LHN_SUM_OUT")):
            return
        cover = {}
        for r in self.recs:
            if r["op"] not in (PW, DW) or isinstance(r["x"], TCat):
                continue
            x = r["x"]
            if self._xs(r)[1] < 2 or (r["op"] == PW and (x.C > 128 or r["out"].C > 128)):
                continue
            spans = cover.setdefault(x.buf, [])
            if any(a < x.coff + x.C and x.coff < b for a, b, _ in spans):
                continue
            spans.append((x.coff, x.coff + x.C, r))
        for b, spans in cover.items():
            spans.sort(key=lambda t: t[0])
            C = self.bufs[b].C
            if spans[0][0] != 0 or spans[-1][1] != C or any(p[1] != q[0] for p, q in zip(spans, spans[1:])):
                continue
            self._sum_written.add(b)
            for lo, hi, r in spans:
                self.sum_out[id(r)] = (self.bufs[b].off["data"], C * 65536 + lo)

    # ------------------------------------------------------------------ forward lowering: one emitter per record family -> [Op]
    def _lower_forward(self):
        emit = {STEM: self._fwd_conv, PW: self._fwd_conv, DW: self._fwd_conv, KXK: self._fwd_conv, PWDW: self._fwd_pwdw, DWPW: self._fwd_dwpw,
                MSRB: self._fwd_msrb, BNECK: self._fwd_bneck, STEMTAIL: self._fwd_stemtail,
                CCW_POOL: self._fwd_ccw, CCW_GATE: self._fwd_ccw, CCW_DW: self._fwd_ccw, CCW_SHUFFLE: self._fwd_ccw,
                FINALIZE: self._fwd_table, TABLE_FILL: self._fwd_table, EW: self._fwd_ew, SHUFFLE: self._fwd_pool,
                MAXPOOL: self._fwd_pool, AVGPOOL: self._fwd_pool, CA_MLP: self._fwd_ca, SE_MLP: self._fwd_se, ATT_MLP: self._fwd_att,
                CBAM: self._fwd_cbam}
        fwd = [self._mk(MEMSET, ws=(self.arena_base["zf"], self.ar["zf"].size))] if self.ar["zf"].size else []
        for r in self.recs:
            fwd += emit[r["op"]](r)
        return fwd

    def _fwd_conv(self, r):
        mk = self._mk
        k, conv, bn, x, out = r["op"], r["conv"], r["bn"], r["x"], r["out"]
        stats = self._abs(r.get("stats"))
        so = self.sum_out.get(id(r), (-1, -1))
        pw = self._p(conv.weight)
        # a trailing BatchNorm rides on the conv op: the last workgroup of the conv finalizes the table
        if bn is not None:
            pbn = self._p_bn(bn)
            wsl = (stats, self._abs(r["save"]), self._abs(r["cnt"]))
            fl = (bn.eps, bn.momentum, r["slope"], float(r.get("bn_repeat", 1)))
        else:
            pbn, wsl, fl = (-1, -1, -1, -1, -1), (stats,), ()
        cb = self._p(getattr(conv, "bias", None)) if bn is not None else -1   # biased conv + BN: bias goes to the finalize
        if k == STEM:
            return [mk(STEM, out=out, p=(pw, cb) + pbn, ws=wsl, i=(r["k"], r["stride"], r["pad"], x.H, x.W), f=fl)]
        if k == KXK:
            return [mk(KXK, ins=(x,), out=out, p=(pw, cb) + pbn, ws=(tuple(wsl) + (-1, -1, -1))[:3] + (self._abs(r["wt"]),),
                       i=(r["stride"], 1) if r.get("bf16x3") else (r["stride"],), f=fl)]
        xv, nx, cf = self._xs(r)
        ws, f = (tuple(wsl) + (-1,) * 4)[:4] + so, (tuple(fl) + (0.0,) * 4)[:4] + tuple(cf)
        if k == PW:
            o = TRef(-1, 0, out.C, out.H, out.W) if r["nchw"] else out
            return [mk(PW, ins=xv, out=o, p=(pw, self._p(conv.bias)) + pbn, ws=ws, f=f,
                       i=(r["stride"], 1 if r["nchw"] else 0, r["wrc"][0], r["wrc"][1], r["stack"][0], r["stack"][1], nx))]
        return [mk(DW, ins=xv, out=out, p=(pw, cb) + pbn, ws=ws, i=(r["k"], r["stride"], r["pad"], r["dil"], 0, 0, nx), f=f)]

    def _fwd_pwdw(self, r):
        return [self._mk(PWDW, ins=(r["x"], r["mid"]), out=r["out"], p=(self._p(r["conv"].weight), self._p(r["conv2"].weight)))]

    def _fwd_dwpw(self, r):
        return [self._mk(DWPW, ins=(r["x"], r["mid"]), out=r["out"], i=(r["dil"],),
                         p=(self._p(r["conv"].weight), self._p(r["conv2"].weight), self._p(r["bias"])))]

    def _fwd_bneck(self, r):
        """in: x and the first two intermediates (tables only); ws[0] = the third intermediate's table, ws[1] = the 3x3's tap-major
        scratch; p = w1, b1, w2, w3, b3 (a bias only where no BatchNorm follows: the unfused 1x1 adds it while storing); f[0] = slope."""
        t1, t2, t3 = r["mids"]
        c1, c2, c3 = r["convs"]
        return [self._mk(BNECK, ins=(r["x"], t1, t2), out=r["out"], ws=(self.bufs[t3.buf].off["table"], self._abs(r["wt"])),
                         p=(self._p(c1.weight), self._p(r["b1"]), self._p(c2.weight), self._p(c3.weight), self._p(r["b3"])), f=(r["slope"],))]

    def _fwd_stemtail(self, r):
        """in: x (K > 0: the depthwise convolution's input; K == 0: t), t and u (tables only); ws[0] = the concatenation buffer's table
        (its first m channels are v's), ws[1] = the 3x3's tap-major scratch; p = w_dw, bT, w1, b1, w2, b2, w3, b3 (-1 = none: see
        fuse_stem); i = K, the table's channel count."""
        c1, c2, c3 = r["convs"]
        cb = self.bufs[r["cat"].buf]
        return [self._mk(STEMTAIL, ins=(r["x"], r["t"], r["u"]), out=r["out"], ws=(cb.off["table"], self._abs(r["wt"])),
                         p=(self._p(r["dw"].weight) if r["dw"] is not None else -1, self._p(r["bT"]), self._p(c1.weight), self._p(r["b1"]),
                            self._p(c2.weight), self._p(r["b2"]), self._p(c3.weight), self._p(r["b3"])), i=(r["K"], cb.C))]

    def _fwd_msrb(self, r):
        """in: the x views of the two halves and the first half's extra source (the second's rides in i[1..3]: an op has three
        input slots); i[0] = OH (0: no pooling), i[6] = sources per half, f[4..5] = their coefficients as on a DW op."""
        two = r["e0"] is not None
        e1 = (r["e1"].buf, r["e1"].coff, r["e1"].C) if two else (-1, 0, 0)
        return [self._mk(MSRB, ins=(r["x0"], r["x1"]) + ((r["e0"],) if two else ()), out=r["out"],
                         p=(self._p(r["conv"].weight), self._p(r["conv2"].weight)), ws=(self._abs(r["pooled"]), self._abs(r["scratch"])),
                         i=(r["OH"],) + e1 + (0, 0, 2 if two else 1), f=(0.0, 0.0, 0.0, 0.0) + tuple(r["coefs"]))]

    def _fwd_ccw(self, r):
        """CCW_GATE: in = pooled, the two 1x1 outputs (tables only), out = g, p = W1, W2, i[0] = mid.  The other three stand behind one
        CCW_ARG op per branch (an op has three input slots and twelve parameters: a block has up to 16 views and 20): in = x2, x1, y,
        out = the shuffled output, p = w_dw, SpatialWeighting's w1, b1, w2, b2, i[0] = its J.  i[0] = B; CCW_POOL: out = pooled;
        CCW_DW: in[0] = g, ws[0] = scratch; CCW_SHUFFLE: ws[0] = scratch."""
        mk = self._mk
        if r["op"] == CCW_GATE:
            return [mk(CCW_GATE, ins=[r["x"]] + r["mids"], out=r["out"], p=(self._p(r["conv"].weight), self._p(r["conv2"].weight)), i=(r["mid"],))]
        args = [mk(CCW_ARG, ins=(x2, x1, y), out=o, p=(self._p(dw.weight),) + tuple(self._p(t) for t in (dn.weight, dn.bias, up.weight, up.bias)), i=(J,))
                for x2, x1, y, o, dw, (dn, up, J) in zip(r["x2"], r["x1"], r["ys"], r["outs"], r["dws"], r["ses"])]
        B = len(args)
        if r["op"] == CCW_POOL:
            return args + [mk(CCW_POOL, out=r["out"], i=(B,))]
        if r["op"] == CCW_DW:
            return args + [mk(CCW_DW, ins=(r["g"],), ws=(self._abs(r["scratch"]),), i=(B,))]
        return args + [mk(CCW_SHUFFLE, ws=(self._abs(r["scratch"]),), i=(B,))]

    def _fwd_table(self, r):
        """FINALIZE: eval-mode table of a convolution that runs inside a PWDW / DWPW / MSRB launch (no statistics to fold); TABLE_FILL: the
        pending bias / activation of a BatchNorm-free convolution."""
        if r["op"] == FINALIZE:
            bn = r["bn"]
            cb = (self._p(r["bias"]),) if r.get("bias") is not None else ()      # p[5]: a convolution bias folded into the shift (fuse_ccw)
            return [self._mk(FINALIZE, out=r["out"], p=self._p_bn(bn) + cb, f=(bn.eps, bn.momentum, r["slope"]))]
        return [self._mk(TABLE_FILL, out=r["out"], p=(self._p(r["bias"]),), i=(1,), f=(1.0, 0.0, r["slope"]))]

    def _fwd_ew(self, r):
        mk = self._mk
        if r.get("lazy") or r.get("fwd_fused"):
            return []
        if "flat" in r:
            # a lazy sum that had to be materialised after all (a reader that cannot add on load): launched on the
            # flattened operand list -- an operand that is itself a lazy sum has never been written
            fl = r["flat"]
            return [mk(EW, ins=[t for t, _ in fl], out=r["out"], i=(len(fl), 1), f=(r["slope"], 0.0, 0.0, 0.0) + tuple(c for _, c in fl))]
        if r.get("mode") or r.get("coefs") is not None:
            cf = r["coefs"] or [1.0] * len(r["srcs"])
            return [mk(EW, ins=r["srcs"], out=r["out"], i=(len(r["srcs"]), 1, r.get("mode", 0)), f=(r["slope"], 0.0, 0.0, 0.0) + tuple(cf))]
        return [mk(EW, ins=r["srcs"], out=r["out"], i=(len(r["srcs"]),), f=(r["slope"],))]

    def _fwd_pool(self, r):
        """Pools and the channel shuffle: data movement without parameters."""
        if r["op"] == SHUFFLE:
            return [self._mk(SHUFFLE, ins=(r["a"], r["b"]), out=r["out"])]
        if r["op"] == MAXPOOL:
            return [self._mk(MAXPOOL, ins=(r["x"],), out=r["out"])]
        ob = self.bufs[r["out"].buf]
        return [self._mk(AVGPOOL, ins=(r["x"],), ws=(ob.off["data"],), i=(r["OH"], r["OW"], 0, ob.C, r["out"].coff))]

    def _fwd_ca(self, r):
        mk = self._mk
        y, ca = r["y"], r["ca"]
        mlp = (self._p(ca.conv1x1[1].weight), self._p(ca.conv1x1[1].bias), self._p(ca.conv1x1[3].weight), self._p(ca.conv1x1[3].bias))
        if hasattr(ca, "rbr_reparam"):
            if self.with_backward:
                raise _lib.LhnError("deployed ChannelAttension is inference-only")
            pool = [] if r.get("pool_fused") else [mk(AVGPOOL, ins=(y,), ws=(self._abs(r["pooled"]),), i=(3, 3, 1))]
            return pool + [mk(CA_MLP, out=y, p=(self._p(ca.rbr_reparam.weight), -1, self._p(ca.rbr_reparam.bias), -1, -1, -1) + mlp,
                              ws=(self._abs(r["pooled"]), self._abs(r["save"]), self._abs(r["mask"])), f=(1e-5, 0.1))]
        sl = r.get("bnslices")
        pins = (y, r["copy"]["srcs"][0]) if r.get("copy") else (y,)       # second input: pass-through half copied by this launch
        if sl:      # pooling pass that also leaves M0, M1 per (n, bin, c) for the backward (lhn_avgpool_fwd4)
            pool = mk(AVGPOOL, ins=pins, ws=(self._abs(r["pooled"]), self._abs(r["pstat"])) + tuple(self._abs(q["save"]) for q in sl),
                      i=(3, 3, 1, 0, 0) + tuple((q["out"].coff << 16) | q["out"].C for q in sl))
        else:
            pool = mk(AVGPOOL, ins=pins, ws=(self._abs(r["pooled"]),), i=(3, 3, 1))
        bn = ca.conv3x3.bn
        return ([] if r.get("pool_fused") else [pool]) + [mk(CA_MLP, out=y, p=(self._p(ca.conv3x3.conv.weight),) + self._p_bn(bn) + mlp,
                         ws=(self._abs(r["pooled"]), self._abs(r["save"]), self._abs(r["mask"]), self._abs(r["gsum"])),
                         f=(bn.eps, bn.momentum))]

    def _fwd_se(self, r):
        y, dn, up = r["y"], r["down"], r["up"]
        pool = [] if r.get("pool_fused") else [self._mk(AVGPOOL, ins=(y,), ws=(self._abs(r["pooled"]),), i=(1, 1, 1))]
        return pool + [self._mk(SE_MLP, out=y, p=(self._p(dn.weight), self._p(dn.bias), self._p(up.weight), self._p(up.bias)),
                                ws=(self._abs(r["pooled"]), self._abs(r["save"])), i=(r["J"], r["mode"]))]

    def _fwd_att(self, r):
        y, att = r["y"], r["att"]
        bn, dw, lin = att[1], att[3], att[6]
        return [self._mk(AVGPOOL, ins=(y,), ws=(self._abs(r["pooled"]),), i=(3, 3, 1)),
                self._mk(ATT_MLP, out=y, p=self._p_bn(bn) + (self._p(dw.weight), self._p(dw.bias), self._p(lin.weight), self._p(lin.bias)),
                         ws=(self._abs(r["pooled"]), self._abs(r["save"]), self._abs(r["mask"]), self._abs(r["gsum"])),
                         f=(bn.eps, bn.momentum))]

    def _cbam_params(self, r):
        m = r["mod"]
        return (self._p(m.ca.sharedMLP[0].weight), self._p(m.ca.sharedMLP[2].weight), self._p(m.sa.conv.weight))

    def _fwd_cbam(self, r):
        return [self._mk(CBAM, ins=(r["p"], r["r"]), out=r["out"], p=self._cbam_params(r), ws=(self._abs(r["save"]),))]

    # ------------------------------------------------------------------ backward lowering
    def _lower_backward(self):
        """The backward op list: the analyses (each one consults the results of those above it), then one emitter per record
        family over the records in REVERSE order -- the emitters share the written-range tracker (_grad_mode / _covered), so
        their order and the order of their tracker calls inside one record decide store against accumulate."""
        self._needs_zero_grad = set()
        self.grad_aliases = self.grad_addends = self.fused_bn_sums = self.reader_bn_sums = self.pool_grad_adds = self.ew_bwd_multi = 0
        for r in self.recs:                     # (not sums_by_ca: the attention record set it while the modules emitted)
            r.pop("sums_by_reader", None)
            r.pop("sums_by_readers", None)
        uses = self._reader_map()
        aliased = self._alias_gradients(uses)
        pending_add = self._grad_addends(uses, aliased)
        fz = _BwdFusions(uses, aliased, pending_add, self._reader_bn_sums(uses, aliased, pending_add))
        fz.fused_mp, fz.skip_ew_src, fz.skip_ap = self._pool_grad_fusion(pending_add, fz.bns_of)
        emit = {STEM: self._bwd_conv, PW: self._bwd_conv, DW: self._bwd_conv, KXK: self._bwd_conv, EW: self._bwd_ew,
                SHUFFLE: self._bwd_shuffle, MAXPOOL: self._bwd_maxpool, AVGPOOL: self._bwd_avgpool,
                CA_MLP: self._bwd_ca, SE_MLP: self._bwd_se, ATT_MLP: self._bwd_att, CBAM: self._bwd_cbam}
        body = []
        for r in reversed(self.recs):
            if r["op"] in (STEM, PW, DW, KXK, EW, SHUFFLE, MAXPOOL, AVGPOOL, CBAM) and not (r["op"] == PW and r.get("nchw")) and \
                    not (self.out_ref is not None and not isinstance(r["out"], TCat) and r["out"].buf == self.out_ref.buf):
                self._covered(fz.written, r["out"])      # (the block output's gradient is written by the engine, not by an op)
            body += emit[r["op"]](r, fz)
        bwd = [self._mk(MEMSET, ws=(self.arena_base["zb"], self.ar["zb"].size))] if self.ar["zb"].size else []
        for b in sorted(self._needs_zero_grad):
            rec = self.bufs[b]
            bwd.append(self._mk(MEMSET, ws=(rec.off["grad"], self.N * rec.H * rec.W * rec.C * 4)))
        self._force_accumulate(body)
        return bwd + body

    def _reader_map(self):
        """buffer -> the records that read it, in record order (one entry per reading view)."""
        uses = {}
        for r in self.recs:
            for t in _reads(r):
                if t.buf >= 0:
                    uses.setdefault(t.buf, []).append(r)
        return uses

    def _alias_gradients(self, uses):
        """Gradient aliasing: a source of a plain (slope 1, same-size, whole-buffer) combine whose ONLY reader is that combine
        receives exactly d(out) -- its gradient buffer becomes an alias of the output's and the copy launch disappears (MSRB:
        the gated branch buffer of every residual add).  Returns the aliased buffers; self._alias_of maps each to its combine's."""
        aliased = set()
        self._alias_of = {}
        for r in reversed(self.recs):
            if r["op"] != EW or r["slope"] != 1.0 or r.get("mode") or r.get("coefs") is not None:
                continue
            out = r["out"]
            ob = self.bufs[out.buf]
            if out.coff != 0 or out.C != ob.C or ob.gate or ob.dpool:
                continue
            for t in r["srcs"]:
                if t.buf < 0 or t.buf == out.buf or t.buf in aliased or len(uses.get(t.buf, ())) != 1:
                    continue
                tb = self.bufs[t.buf]
                if (self.in_ref is not None and t.buf == self.in_ref.buf) or t.coff != 0 or t.C != tb.C:
                    continue
                if (t.H, t.W) != (out.H, out.W) or sum(1 for q in r["srcs"] if q.buf == t.buf) != 1:
                    continue
                tb.off["grad"] = ob.off["grad"]
                aliased.add(t.buf)
                self._alias_of[t.buf] = out.buf
        self.grad_aliases = len(aliased)
        return aliased

    def _grad_addends(self, uses, aliased):
        """Gradient addends: a plain residual sum O = S + ... hands d(O) to every source.  When S's other readers are
        tiled depthwise convolutions whose input slices tile S exactly (MSRB: `out` feeds the two dilated 3x3 halves
        and the running sum, litehourglass.py:41-49), those convolutions' backward kernels add d(O) while storing
        their dx (include/lhn.h: lhn_conv_dw_bwd3) and the sum's copy / accumulate pass over S's gradient disappears.
        Returns S's buffer -> [(id(sum record), O's buffer, channel shift)]."""
        pending_add = {}
        if not _switch("LHN_GRAD_ADDENDS"):
            return pending_add
        order = {id(q): j for j, q in enumerate(self.recs)}

        def plain_sum(q):
            return q["op"] == EW and q["slope"] == 1.0 and not q.get("mode") and q.get("coefs") is None and \
                not isinstance(q["out"], TCat)

        for sb, rd in uses.items():
            if sb in aliased or sb == self._no_grad_buf:
                continue
            sums = [q for q in rd if plain_sum(q)]
            dws = [q for q in rd if not plain_sum(q)]
            if not sums or not dws or len(sums) > 2:
                continue
            if not all(q["op"] == DW and q["conv"].weight is not None and q["stride"] == 1 and q["k"] == 3 and
                       q["pad"] == q["dil"] and q["x"].C % 32 == 0 and q["x"].W >= 8 and not isinstance(q["x"], TCat)
                       for q in dws):
                continue
            if min(order[id(q)] for q in sums) < max(order[id(q)] for q in dws):
                continue
            spans = sorted((q["x"].coff, q["x"].coff + q["x"].C) for q in dws)
            lo, hi = spans[0][0], spans[-1][1]
            if any(a[1] != b[0] for a, b in zip(spans, spans[1:])):
                continue
            adds = []
            for q in sums:
                mine = [t for t in q["srcs"] if not isinstance(t, TCat) and t.buf == sb]
                o = q["out"]
                if len(mine) != 1 or (mine[0].coff, mine[0].C) != (lo, hi - lo) or (mine[0].H, mine[0].W) != (o.H, o.W) or \
                        self.bufs[o.buf].C != self.bufs[sb].C:
                    break
                adds.append((id(q), o.buf, o.coff - lo))
            else:
                pending_add[sb] = adds
        return pending_add

    @staticmethod
    def _can_add_bn_sums(q, t, pending_add):
        """True when the backward kernel of reader record q can add its part of the BatchNorm-backward sums for its input view t."""
        if q["op"] == EW:
            return not q.get("lazy") and "flat" not in q and not q.get("mode") and q.get("coefs") is None and \
                q["slope"] not in (SLOPE_SILU, SLOPE_RELU_SIGMOID) and not isinstance(q["out"], TCat) and \
                not any(a[0] == id(q) for a in pending_add.get(t.buf, ())) and \
                q["out"].H % t.H == 0 and q["out"].W % t.W == 0
        if q["op"] == PW:
            # (which shapes have a backward kernel that takes the sums is the library's answer: lhn_conv_pw_route, feature 64 =
            # LHN_PW_F_BNSUM, the switches as the process read them -- the answer does not depend on them)
            return not q.get("nchw") and q.get("xs") is None and not q["wrc"][1] and not q["wrc"][0] and \
                (t.coff, t.C) == (q["x"].coff, q["x"].C) and \
                _lib.lib().lhn_conv_pw_route(1, 1, t.H, t.W, t.C, q["out"].C, q["stride"], 0, 0, 64, -1) is not None
        return q["op"] in (MAXPOOL, AVGPOOL)

    def _reader_bn_sums(self, uses, aliased, pending_add):
        """Reader-side BatchNorm sums, general form (include/lhn.h: lhn_bnsum): du is linear in dz and dz is the sum of what the
        readers' backward kernels hand back, so when EVERY reader of a convolution + BatchNorm output can add its part
        (elementwise combines, pools, the fused 1x1 backward) the producer's lhn_bn_bwd_reduce pass is not launched: the
        producer record gets sums_by_readers.  Returns (id(reader record), buf, coff, C) of every such reading view ->
        ((sums, save) offsets of the producer, (the producer's C, the view's channel offset inside it))."""
        bns = {}
        if not _switch("LHN_READER_BN_SUMS"):
            return bns
        for P in self.recs:
            if P["op"] not in (STEM, PW, DW, KXK) or P["bn"] is None or P.get("sums_by_ca") or isinstance(P["out"], TCat):
                continue
            o = P["out"]
            if o.buf < 0 or P.get("wrc", (0, 0))[0] or P.get("bn_repeat", 1) != 1 or o.buf in aliased:
                continue
            ob = self.bufs[o.buf]
            if ob.gate or ob.dpool or ob.lazy is not None or (self.out_ref is not None and o.buf == self.out_ref.buf):
                continue
            lo, hi = o.coff, o.coff + o.C
            mine, ok = [], True
            for q in uses.get(o.buf, ()):
                for t in _reads(q):
                    if t.buf != o.buf or t.coff + t.C <= lo or hi <= t.coff:
                        continue
                    ok = ok and lo <= t.coff and t.coff + t.C <= hi and self._can_add_bn_sums(q, t, pending_add)
                    mine.append((q, t))
            if ok and mine:
                P["sums_by_readers"] = True
                self.reader_bn_sums += 1
                for q, t in mine:
                    bns[(id(q), t.buf, t.coff, t.C)] = ((self._abs(P["sums"]), self._abs(P["save"])), (o.C, t.coff - lo))
        return bns

    def _pool_grad_fusion(self, pending_add, bns_of):
        """Readers of one tensor whose gradients meet in ONE store (lhn_grad_adds): a 2x2 max-pool, an adaptive average pool
        and a plain same-resolution sum reading the same view (the skip tensor of an hourglass level, litehourglass.py:139-163)
        -- the max-pool's backward, which runs last, takes the other two gradients on the way (LHN_POOL_GRAD_ADDS=0: three
        read-modify-write passes over d(x) as before).  Returns (id(max-pool record) -> ((sum record, source index) | None,
        average-pool record | None), the (id(sum record), source index) pairs and the id(average-pool record)s taken over)."""
        fused_mp, skip_ew_src, skip_ap = {}, set(), set()
        if not _switch("LHN_POOL_GRAD_ADDS"):
            return fused_mp, skip_ew_src, skip_ap
        order = {id(q): i for i, q in enumerate(self.recs)}
        for mp in self.recs:
            if mp["op"] != MAXPOOL or isinstance(mp["x"], TCat) or mp["x"].H % 2 or mp["x"].W % 2 or mp["x"].buf == self._no_grad_buf:
                continue
            X = mp["x"]

            def same(t, X=X):
                return not isinstance(t, TCat) and t.buf == X.buf and t.coff == X.coff and t.C == X.C
            ap = next((q for q in self.recs if q["op"] == AVGPOOL and "OH" in q and same(q["x"]) and order[id(q)] > order[id(mp)]
                       and id(q) not in skip_ap), None)
            ew = None
            for q in self.recs:
                if q["op"] != EW or q.get("lazy") or q.get("fwd_fused") or "flat" in q or q.get("mode") or q.get("coefs") is not None:
                    continue
                if order[id(q)] < order[id(mp)] or float(q["slope"]) != 1.0 or isinstance(q["out"], TCat):
                    continue
                ob = self.bufs[q["out"].buf]
                idx = [j for j, t in enumerate(q["srcs"]) if same(t)]
                if ob.gate or ob.dpool or len(idx) != 1 or (q["srcs"][idx[0]].H, q["srcs"][idx[0]].W) != (q["out"].H, q["out"].W):
                    continue
                if (id(q), idx[0]) in skip_ew_src or any(a[0] == id(q) for a in pending_add.get(X.buf, ())):
                    continue
                ew = (q, idx[0])
                break
            if ap is None and ew is None:
                continue
            keys = [bns_of(mp, X)] + ([bns_of(ap, X)] if ap else []) + ([bns_of(ew[0], X)] if ew else [])
            if any(kk != keys[0] for kk in keys):      # the producer's BatchNorm sums: all of x's readers or none
                continue
            fused_mp[id(mp)] = (ew, ap)
            if ew:
                skip_ew_src.add((id(ew[0]), ew[1]))
            if ap:
                skip_ap.add(id(ap))
        self.pool_grad_adds = len(fused_mp)
        return fused_mp, skip_ew_src, skip_ap

    # ---- backward emitters: (record, _BwdFusions) -> [Op]
    def _bwd_conv(self, r, fz):
        mk = self._mk
        k, conv, bn, x, out = r["op"], r["conv"], r["bn"], r["x"], r["out"]
        pw = self._p(conv.weight)
        use_coef = 1 if bn is not None else 0
        ops = []
        lz = self.bufs[x.buf].lazy if x.buf >= 0 else None
        if lz is not None and x.buf not in fz.materialised and x.buf not in self._sum_written:
            # the weight gradient needs the summed input: written once per backward, whole buffer
            fz.materialised.add(x.buf)
            fl = lz["flat"]
            ops.append(mk(EW, ins=[t for t, _ in fl], out=lz["out"], i=(len(fl), 1), f=(1.0, 0.0, 0.0, 0.0) + tuple(c for _, c in fl)))
        if bn is not None:      # (sums_by_reader: set by the depthwise reader's emitter, which ran before this one -- see _bwd_dw)
            by_others = r.get("sums_by_reader") or r.get("sums_by_ca") or r.get("sums_by_readers")
            ops.append(mk(BN_BWD, out=out, p=(self._p(bn.weight), self._p(bn.weight), self._p(bn.bias)),
                          ws=(self._abs(r["sums"]), self._abs(r["save"]), self._abs(r["bcnt"])),
                          i=(r["wrc"][0] if k == PW else 0, 1 if by_others else 0)))
        if k == STEM:
            return ops + [mk(STEM_BWD, out=out, p=(pw, pw), i=(r["k"], r["stride"], r["pad"], x.H, x.W, use_coef))]
        need_dx = x.buf != self._no_grad_buf
        mode = self._grad_mode(fz.written, x) if need_dx else 0
        if k == PW:
            if r["stride"] != 1 and mode == 1:   # strided dgrad touches a subset of pixels
                self._needs_zero_grad.add(x.buf)
                mode = 2
            o = TRef(-1, 0, out.C, out.H, out.W) if r["nchw"] else out
            # a bias in front of a train-mode BatchNorm has an identically zero gradient
            bw, bc = fz.bns_of(r, x) if need_dx else ((-1, -1), (0, 0))
            ops.append(mk(PW_BWD, ins=(x,), out=o, p=(pw, pw, self._p(conv.bias) if bn is None else -1), ws=bw,
                          i=(r["stride"], 1 if r["nchw"] else 0, mode, r["wrc"][0], r["wrc"][1], use_coef,
                             r["stack"][0], r["stack"][1]), f=(0.0,) * 6 + (float(bc[0]), float(bc[1]))))
        elif k == DW:
            ops.append(self._bwd_dw(r, mode, need_dx, fz))
        else:
            ops.append(mk(KXK_BWD, ins=(x,), out=out, p=(pw, pw), ws=(-1, -1, -1, self._abs(r["wt"])),
                          i=(r["stride"], 0, mode, 0, 0, use_coef)))
        return ops

    def _sole_reader_producer(self, r, mode, fz):
        """The convolution + BatchNorm record whose output is exactly the input view of depthwise record r, when r is that
        buffer's only reader and stores its dx (mode 1) with the 3x3 stride-1 kernel -- or None."""
        x, xb = r["x"], self.bufs[r["x"].buf]
        if not (_switch("LHN_FUSE_BN_SUMS") and mode == 1 and r["k"] == 3 and r["stride"] == 1 and r["pad"] == 1 and r["dil"] == 1 and
                x.C % 32 == 0 and x.W >= 8 and not xb.gate and not xb.dpool and xb.lazy is None and
                r["conv"].weight is not None and len(fz.uses.get(x.buf, ())) == 1 and x.buf not in fz.aliased):
            return None
        prod = None
        for q in self.recs:
            if q["op"] in (STEM, PW, DW, KXK) and q["bn"] is not None and q["out"].buf == x.buf and \
                    (q["out"].coff, q["out"].C) == (x.coff, x.C) and not q.get("wrc", (0, 0))[0] and q.get("bn_repeat", 1) == 1:
                prod = q
        return prod

    def _bwd_dw(self, r, mode, need_dx, fz):
        """The DW_BWD op of depthwise record r.  It carries the gradient addends of its input buffer (fz.pending_add), or else
        the BatchNorm-backward sums of its input's producer when it is the only reader of x (RepBasicUnit 1x1 -> 3x3 depthwise;
        include/lhn.h: lhn_conv_dw_bwd2).  The second is decided HERE, not in an analysis, because it depends on the store mode
        the tracker just returned: the producer gets sums_by_reader, which its own BN_BWD op -- emitted later, the records
        being walked in reverse -- reads in _bwd_conv."""
        x, pw = r["x"], self._p(r["conv"].weight)
        geo = (r["k"], r["stride"], r["pad"], r["dil"], mode, 1 if r["bn"] is not None else 0)
        adds = fz.pending_add.get(x.buf)
        if adds and need_dx:
            self.grad_addends += 1
            offs = [self.bufs[ob].off["grad"] + 4 * sh for _, ob, sh in adds]
            return self._mk(DW_BWD, ins=(x,), out=r["out"], p=(pw, pw), ws=(-1, -1, offs[0], offs[1] if len(offs) > 1 else -1), i=geo)
        prod = self._sole_reader_producer(r, mode, fz)
        if prod is None:
            return self._mk(DW_BWD, ins=(x,), out=r["out"], p=(pw, pw), i=geo)
        prod["sums_by_reader"] = True
        self.fused_bn_sums += 1
        return self._mk(DW_BWD, ins=(x,), out=r["out"], p=(pw, pw), ws=(-1, -1, -1, -1, self._abs(prod["sums"]), self._abs(prod["save"])),
                        i=geo + (x.C, 0))

    def _bwd_ew_mode(self, r, fz):
        """Products, bilinear resampling and combines with coefficients: one op per source."""
        md, srcs, ops = r.get("mode", 0), r["srcs"], []
        if r.get("coefs") is not None and any(c != 1.0 for c in r["coefs"]):
            raise _lib.LhnError("a combine with coefficients is forward-only")
        if (md & EW_MUL) and r["slope"] != 1.0:
            raise _lib.LhnError("a product combine with an output activation is forward-only (lhn_ew_mul_bwd takes no slope)")
        for j, s in enumerate(srcs):
            if s.buf == self._no_grad_buf:
                continue
            acc = 1 if self._grad_mode(fz.written, s) == 2 else 0
            if md & EW_MUL:
                ops.append(self._mk(EW_BWD, ins=(s, srcs[1 - j]), out=r["out"], i=(acc, 1), f=(r["slope"],)))
            elif (md & EW_BILINEAR) and (s.H, s.W) != (r["out"].H, r["out"].W):
                ops.append(self._mk(EW_BWD, ins=(s,), out=r["out"], i=(acc, 2), f=(r["slope"],)))
            else:
                ops.append(self._mk(EW_BWD, ins=(s,), out=r["out"], i=(acc,), f=(r["slope"],)))
        return ops

    @staticmethod
    def _multi_groups(r, todo):
        """Sources of the destination's own resolution (residual sums) share ONE pass over d(out) / out (lhn_ew_bwd_multi): the
        (source, accumulate, sums ws, sums (C, coff)) entries of `todo` in groups of 2 or 3, or [] (LHN_EW_BWD_MULTI=0)."""
        o = r["out"]
        same = [t for t in todo if not isinstance(t[0], TCat) and (t[0].H, t[0].W, t[0].C) == (o.H, o.W, o.C)]
        if not _switch("LHN_EW_BWD_MULTI") or len(same) < 2 or r["slope"] in (SLOPE_SILU, SLOPE_RELU_SIGMOID):
            return []
        groups = []
        while len(same) >= 2:
            take = 3 if len(same) != 4 else 2
            groups.append(same[:take])
            same = same[take:]
        return groups

    def _bwd_ew(self, r, fz):
        if r.get("mode") or r.get("coefs") is not None:
            return self._bwd_ew_mode(r, fz)
        todo = []
        for j, s in enumerate(r["srcs"]):
            if s.buf == self._no_grad_buf or (s.buf in fz.aliased and self.bufs[s.buf].off["grad"] == self.bufs[r["out"].buf].off["grad"]):
                continue
            if (id(r), j) in fz.skip_ew_src:
                continue                # d(out) joins s's gradient inside the max-pool backward that reads s (fused_mp)
            if any(a[0] == id(r) for a in fz.pending_add.get(s.buf, ())):
                continue                # d(out) joins s's gradient inside the depthwise backward kernels that read s
            mode = self._grad_mode(fz.written, s)
            todo.append((s, 1 if mode == 2 else 0) + fz.bns_of(r, s))
        groups = self._multi_groups(r, todo)        # (after every tracker call of this record)
        self.ew_bwd_multi += len(groups)
        ops = []
        for g in groups:
            g3 = g + [(None, 0, (-1, -1), (0, 0))] * (3 - len(g))
            ops.append(self._mk(EW_BWD, ins=tuple(t[0] for t in g), out=r["out"], ws=g3[0][2] + g3[1][2] + g3[2][2],
                                i=(g3[0][1], 3, g3[1][1], g3[2][1]) + g3[0][3] + g3[1][3],
                                f=(r["slope"], 0.0, 0.0, 0.0, float(g3[2][3][0]), float(g3[2][3][1]))))
        grouped = {id(t[0]) for g in groups for t in g}
        ops += [self._mk(EW_BWD, ins=(s,), out=r["out"], ws=bw, i=(acc, 0, 0, 0, bc[0], bc[1]), f=(r["slope"],))
                for s, acc, bw, bc in todo if id(s) not in grouped]
        return ops

    def _bwd_shuffle(self, r, fz):
        ma = 0 if r["a"].buf == self._no_grad_buf else self._grad_mode(fz.written, r["a"])
        mb = 0 if r["b"].buf == self._no_grad_buf else self._grad_mode(fz.written, r["b"])
        return [self._mk(SHUFFLE_BWD, ins=(r["a"], r["b"]), out=r["out"], i=(ma, mb))]

    def _bwd_maxpool(self, r, fz):
        mode = self._grad_mode(fz.written, r["x"])
        bw, bc = fz.bns_of(r, r["x"])
        ew, ap = fz.fused_mp.get(id(r), (None, None))
        sw, si, pw_, pi = -1, (0, 0), -1, (0, 0, 0)
        if ew is not None:
            eo = ew[0]["out"]
            sw, si = self.bufs[eo.buf].off["grad"], (self.bufs[eo.buf].C, eo.coff)
        if ap is not None:
            ob = self.bufs[ap["out"].buf]
            pw_, pi = ob.off["grad"], (ob.C, ap["out"].coff, (ap["OH"] << 16) | ap["OW"])
        return [self._mk(MAXPOOL_BWD, ins=(r["x"],), out=r["out"], ws=bw + (sw, pw_),
                         i=(1 if mode == 2 else 0, si[0], si[1], pi[0], bc[0], bc[1], pi[1], pi[2]))]

    def _bwd_avgpool(self, r, fz):
        if id(r) in fz.skip_ap:
            return []                   # its gradient joins d(x) inside the max-pool backward (fused_mp)
        mode = self._grad_mode(fz.written, r["x"])
        ob = self.bufs[r["out"].buf]
        bw, bc = fz.bns_of(r, r["x"])
        return [self._mk(AVGPOOL_BWD, ins=(r["x"],), ws=(ob.off["grad"],) + bw,
                         i=(r["OH"], r["OW"], 1 if mode == 2 else 0, ob.C, r["out"].coff, bc[0], bc[1]))]

    def _bwd_se(self, r, fz):
        y, dn, up, P = r["y"], r["down"], r["up"], self._p
        return [self._mk(GATE_REDUCE, out=y, ws=(-1, -1, -1, self._abs(r["dgate"]))),
                self._mk(SE_MLP_BWD, out=y, p=(P(dn.weight), P(up.weight), P(dn.weight), P(dn.bias), P(up.weight), P(up.bias)),
                         ws=(self._abs(r["pooled"]), self._abs(r["save"]), -1, self._abs(r["dgate"])), i=(r["J"], r["mode"]))]

    def _bwd_cbam(self, r, fz):
        """d(p) and d(r) are stored: the CBAM record is the only reader of both buffers (cbam_attention made them)."""
        for t in (r["p"], r["r"]):
            if self._grad_mode(fz.written, t) != 1:
                raise _lib.LhnError("CBAM backward stores the gradients of its two inputs: they must have no other reader")
        pp = self._cbam_params(r)
        return [self._mk(CBAM_BWD, ins=(r["p"], r["r"]), out=r["out"], p=pp + pp, ws=(self._abs(r["save"]), self._abs(r["scratch"])))]

    def _bwd_att(self, r, fz):
        y, att, P = r["y"], r["att"], self._p
        bn, dw, lin = att[1], att[3], att[6]
        return [self._mk(GATE_REDUCE, out=y, ws=(-1, -1, -1, self._abs(r["dgate"]))),
                self._mk(ATT_MLP_BWD, out=y, p=(P(bn.weight), P(bn.bias), P(dw.weight), P(lin.weight),
                                                P(bn.weight), P(bn.bias), P(dw.weight), P(dw.bias), P(lin.weight), P(lin.bias)),
                         ws=tuple(self._abs(r[key]) for key in ("pooled", "save", "mask", "dgate", "gsum_b")))]

    def _bwd_ca(self, r, fz):
        y, ca, P = r["y"], r["ca"], self._p
        c3, bn, l1, l2 = ca.conv3x3.conv, ca.conv3x3.bn, ca.conv1x1[1], ca.conv1x1[3]
        sl = r.get("bnslices") or []
        pk = tuple((q["out"].coff << 16) | q["out"].C for q in sl)
        sv = (tuple(self._abs(q["save"]) for q in sl) + (-1, -1))[:2]
        sm = (tuple(self._abs(q["sums"]) for q in sl) + (-1, -1))[:2]
        return [self._mk(GATE_REDUCE, out=y, ws=(-1, -1, -1, self._abs(r["dgate"]), 1 if sl else -1) + sv, i=pk),
                self._mk(CA_MLP_BWD, out=y, p=(P(c3.weight), P(bn.weight), P(l1.weight), P(l2.weight), P(c3.weight), P(bn.weight), P(bn.bias),
                                               P(l1.weight), P(l1.bias), P(l2.weight), P(l2.bias)),
                         ws=tuple(self._abs(r.get(key)) for key in ("pooled", "save", "mask", "dgate", "gsum_b", "pstat")) + sv + sm, i=pk)]

    # gradient-write slot of a backward op and the value that means "accumulate": mode slots (0 none, 1 store, 2 accumulate)
    # are only raised when set, flag slots are set
    _ACCUMULATE = {PW_BWD: (2, 2), KXK_BWD: (2, 2), DW_BWD: (4, 2), EW_BWD: (0, 1), MAXPOOL_BWD: (0, 1), AVGPOOL_BWD: (2, 1)}

    def _force_accumulate(self, body):
        """Every write into a zero-initialised gradient buffer (_needs_zero_grad, complete only after the emitters ran) must accumulate."""
        zg = self._needs_zero_grad
        for o in (body if zg else ()):
            if o.kind == SHUFFLE_BWD:
                for q in range(2):
                    if o.in_buf[q] in zg and o.i[q]:
                        o.i[q] = 2
            elif o.kind in self._ACCUMULATE and o.in_buf[0] in zg:
                slot, acc = self._ACCUMULATE[o.kind]
                if acc == 1 or o.i[slot]:
                    o.i[slot] = acc

    @staticmethod
    def _sync_points(fwd, bwd):
        """SyncBatchNorm: (op index, byte offset, number of doubles, replicated layout?) of every statistics buffer that has to be
        all-reduced between half-step 2*i and 2*i+1 of lhn_plan_run_range, per phase."""
        pts = {0: [], 1: []}
        for lst in (fwd, bwd):
            for i, o in enumerate(lst):
                if o.kind in (STEM, PW, DW, KXK) and o.p[2] >= 0 and o.ws[0] >= 0:
                    pts[0].append((i, o.ws[0], STAT_REPLICAS * 2 * o.out_C, True))
                elif o.kind in (CA_MLP, ATT_MLP) and o.ws[3] >= 0:
                    pts[0].append((i, o.ws[3], 2 * o.out_C, False))
                elif o.kind == BN_BWD:
                    pts[1].append((i, o.ws[0], STAT_REPLICAS * 2 * o.out_C, True))
                elif o.kind in (CA_MLP_BWD, ATT_MLP_BWD) and o.ws[4] >= 0:
                    pts[1].append((i, o.ws[4], 2 * o.out_C, False))
        return pts

    def _c_arrays(self, fwd, bwd):
        cb = (Buf * len(self.bufs))()
        for j, b in enumerate(self.bufs):
            cb[j].data_off = b.off["data"]
            cb[j].table_off = b.off["table"]
            cb[j].gate_off = b.off.get("gate", -1)
            cb[j].grad_off = b.off.get("grad", -1)
            cb[j].dpool_off = b.off.get("dpool", -1)
            cb[j].coef_off = b.off.get("coef", -1)
            cb[j].N, cb[j].H, cb[j].W, cb[j].C = self.N, b.H, b.W, b.C
        cf = (Op * len(fwd))(*fwd)
        cbw = (Op * max(1, len(bwd)))(*bwd) if bwd else None
        return cb, cf, cbw, len(fwd), len(bwd)


_SIDE_STREAMS = {}


def _graph_default(n_ops):
    """hipGraph replay of a plan's launch sequence (LHN_RUN_GRAPH): only with LHN_GRAPH=1.  Measured on MI355X (round 3, same
    box, Lite-HRNet-18 at batch 64, 663 forward ops / 2,600 launches per step): replay 38.83 ms per step and 13.22 ms per
    forward against 37.16 / 12.43 ms with plain launches -- outside the profiler the host keeps up with the queue, and a
    graph launch adds its fixed cost per phase.  So replay is NOT a default for any plan size."""
    return os.environ.get("LHN_GRAPH", "") == "1"


def _side_stream(device):
    """One non-default stream per device: the legacy default stream cannot be captured into a hipGraph."""
    key = torch.device(device).index
    s = _SIDE_STREAMS.get(key)
    if s is None:
        s = _SIDE_STREAMS[key] = torch.cuda.Stream(device=device)
    return s


_TRAIN_RUNS = 0      # bumped by every train-mode forward of any plan in this process (see CompiledPlan.run)
_TABLE_EPOCH = 0     # bumped by invalidate_tables(): state changed where neither torch's version counters nor data pointers see it


def invalidate_tables():
    """Every plan's cached eval-mode BatchNorm tables / deployed biases become stale.  Call after changing parameters or
    running statistics through `.data` (p.data.mul_(..), EMA / weight surgery): such writes bump no version counter.
    litehandnet_amd.train.Trainer.step and FlatParams.broadcast call it themselves."""
    global _TABLE_EPOCH
    _TABLE_EPOCH += 1


class CompiledPlan:
    """Owns the C plan + the workspace arena (a torch uint8 tensor) for one (module, input shape)."""

    def __init__(self, pb: PlanBuilder, state_tensors, device):
        self.pb = pb
        cb, cf, cbw, nf, nb = pb.finalize()
        self._keep = (cb, cf, cbw)
        L = _lib.lib()
        self.handle = L.lhn_plan_create(cb, len(pb.bufs), cf, nf, cbw, nb)
        if not self.handle:
            raise _lib.LhnError("lhn_plan_create: " + L.lhn_last_error().decode())
        self.n_fwd, self.n_bwd = nf, nb
        self.use_graph = _graph_default(nf)
        self.ws = torch.empty(pb.total_bytes, dtype=torch.uint8, device=device)
        # tables start as the identity transform (scale 1, shift 0, slope 1); FINALIZE overwrites BN slices
        for b in pb.bufs:
            t = self.view_f32(b.off["table"], 3 * b.C).view(3, b.C)
            t[0].fill_(1.0)
            t[1].zero_()
            t[2].fill_(1.0)
            if "coef" in b.off:     # dy = A du + B y + C: identity until a BatchNorm backward writes its slice (padded
                c = self.view_f32(b.off["coef"], 3 * b.C).view(3, b.C)      # channels of a 7 / 17 / 37-wide one never are)
                c[0].fill_(1.0)
                c[1].zero_()
                c[2].zero_()
        self.state_tensors = state_tensors
        self._params = (C.c_void_p * len(state_tensors))()
        self._grads = (C.c_void_p * len(state_tensors))()
        self._io = (C.c_void_p * 2)()
        self._table_sig = None
        self.fwd_serial = 0            # forwards run on this workspace so far
        self.bwd_serial = -1           # serial of the forward whose backward has already consumed the workspace
        self.mask_view = None
        # dropout masks (Dropout2d of ChannelAttension, common.py:57; Dropout of mynet's attention, pose_hg_ms_att.py:171):
        # one [N, C] slice per attention module, values 0 or 1/keep.  `mask_fn(plan)`, when set, fills them instead of the
        # default bernoulli_ draw -- parity tests feed the oracle the same masks.
        self.mask_fn = None            # plan-level override; otherwise the owning engine's `mask_fn` as it is at run time
        self.engine = None
        self.mask_slices = []
        if pb.ar["mask"].size:
            self.mask_view = self.view_f32(pb.arena_base["mask"], pb.ar["mask"].size // 4)
            for r in pb.recs:
                if r.get("mask") is not None:
                    mod = r.get("ca", r.get("att"))
                    Cc = r["y"].C
                    self.mask_slices.append((mod, self.view_f32(pb._abs(r["mask"]), pb.N * Cc).view(pb.N, Cc)))

    def view_f32(self, byte_off, numel):
        return self.ws[byte_off:byte_off + numel * 4].view(torch.float32)

    def buf_data(self, ref, grad=False):
        b = self.pb.bufs[ref.buf]
        v = self.view_f32(b.off["grad" if grad else "data"], self.pb.N * b.H * b.W * b.C)
        return v.view(self.pb.N, b.H, b.W, b.C)[..., ref.coff:ref.coff + ref.C]

    def refresh_params(self):
        for j, t in enumerate(self.state_tensors):
            self._params[j] = t.data_ptr()

    def set_grads(self, grad_tensors):
        for j, g in enumerate(grad_tensors):
            self._grads[j] = 0 if g is None else g.data_ptr()

    def run(self, phase, io0, io1, training, grad_replicas=1, grad_rep_stride=0, sync=None):
        """sync = (world, all_reduce_fn) runs the phase in SyncBatchNorm mode: the launch sequence is cut at every
        statistics buffer, `all_reduce_fn(float64 view)` sums it over the ranks, statistics count N*world samples."""
        self._io[0] = 0 if io0 is None else io0.data_ptr()
        self._io[1] = 0 if io1 is None else io1.data_ptr()
        global _TRAIN_RUNS
        if phase == 0:
            self.fwd_serial += 1       # the workspace (activations, BatchNorm saves, masks, gates) now belongs to THIS forward
        if phase == 0 and training:
            _TRAIN_RUNS += 1           # running statistics are about to move: every plan's eval tables become stale
            self._table_sig = None
        if phase == 0 and training and self.mask_view is not None:
            fn = self.mask_fn if self.mask_fn is not None else getattr(self.engine, "mask_fn", None)
            if fn is not None:
                fn(self)
            else:
                keep = 1.0 - self.pb.p_drop
                self.mask_view.bernoulli_(keep).mul_(1.0 / keep)
        L = _lib.lib()
        if sync is not None and training and sync[0] > 1:
            world, allreduce = sync
            nsteps = 2 * (self.n_fwd if phase == 0 else self.n_bwd)

            def run_range(b, e):
                rc = L.lhn_plan_run_range(C.c_void_p(self.handle), phase, C.c_int64(b), C.c_int64(e), _lib.ptr(self.ws),
                                          self._params, self._grads, self._io, 1, int(grad_replicas),
                                          C.c_int64(int(grad_rep_stride)), C.c_double(float(world)), C.c_float(1.0 / world),
                                          _lib.stream())
                _lib.check(rc, "lhn_plan_run_range")
            begin = 0
            self.sync_wire_doubles = 0
            for oi, off, n, replicated in self.pb.sync_points[phase]:
                run_range(begin, 2 * oi + 1)
                if replicated:
                    # replicated [32][2][C] sums: folded on the device first, only [2][C] doubles cross the wire
                    m = n // STAT_REPLICAS
                    _lib.check(L.lhn_fold_stat_replicas(C.c_void_p(self.ws.data_ptr() + off), C.c_int64(m), STAT_REPLICAS, _lib.stream()),
                               "lhn_fold_stat_replicas")
                    n = m
                allreduce(self.ws[off:off + 8 * n].view(torch.float64))
                self.sync_wire_doubles += n
                begin = 2 * oi + 1
            run_range(begin, nsteps)
            return
        mode = 1 if training else 0
        if phase == 0:
            # eval-mode BatchNorm tables / deployed biases only depend on the parameters: rebuild them when something changed
            # (torch's per-tensor version counters catch load_state_dict / optimizer steps; our own train-mode kernels update
            # running statistics behind torch's back, so any training run anywhere invalidates every plan's tables)
            if not training and self._tables_current():
                mode |= 2              # LHN_RUN_TABLES_CURRENT
        if self.use_graph:
            # replayed as a hipGraph (LHN_RUN_GRAPH).  On torch's default stream -- which cannot be captured -- the phase runs
            # on a side stream ordered after everything queued so far, and the default stream waits for it: the caller sees
            # the usual stream semantics (no exec, no capture of the default stream).
            cur = torch.cuda.current_stream(self.ws.device)
            if cur.cuda_stream == 0:
                side = _side_stream(self.ws.device)
                side.wait_stream(cur)
                rc = L.lhn_plan_run(C.c_void_p(self.handle), phase, _lib.ptr(self.ws), self._params, self._grads, self._io,
                                    mode | 4, int(grad_replicas), C.c_int64(int(grad_rep_stride)), C.c_void_p(side.cuda_stream))
                cur.wait_stream(side)
                _lib.check(rc, "lhn_plan_run")
                return
            mode |= 4
        rc = L.lhn_plan_run(C.c_void_p(self.handle), phase, _lib.ptr(self.ws), self._params, self._grads, self._io,
                            mode, int(grad_replicas), C.c_int64(int(grad_rep_stride)), _lib.stream())
        _lib.check(rc, "lhn_plan_run")

    def _tables_current(self):
        """True when this eval run may reuse the tables the previous eval run of this plan built.  Remembers the state it
        saw: (process-wide count of train-mode runs, the invalidate_tables() epoch, torch's version counter and the data
        pointer of every parameter / buffer).  Tensors without a version counter (created under torch.inference_mode)
        disable the reuse.  Writes through `.data` are invisible to all of these: see invalidate_tables()."""
        try:
            sig = (_TRAIN_RUNS, _TABLE_EPOCH, tuple(t._version for t in self.state_tensors),
                   tuple(t.data_ptr() for t in self.state_tensors))
        except RuntimeError:
            self._table_sig = None
            return False
        same = sig == self._table_sig
        self._table_sig = sig
        return same

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                _lib.lib().lhn_plan_destroy(C.c_void_p(self.handle))
                self.handle = None
        except Exception:
            pass
