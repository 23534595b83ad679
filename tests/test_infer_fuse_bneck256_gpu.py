"""GPU: the BottleNeck inference fusion (plan.set_infer_fuse_bneck) through the plan executor at 256 channels: 256 -> 64 -> 256 and
256 -> 128 -> 256 blocks each run as one launch (lhn_bottleneck_fwd).

Variant A itself does not run on the GPU at channels=256: every Residual starts with a BasicBlock whose dense 3x3 is 256 -> 256, and
lhn_conv_kxk_fwd is built for at most 128 channels ("unsupported channels Cin=256 Cout=256", with the fusion on or off).  So the
network here is `Hourglass256`: the thirteen BottleNecks of variant A's hourglass and neck at width 256, on the maps a 64 x 64 image
gives them (two at 8 x 8, four at 4 x 4, six at 2 x 2, the neck's `reduction=2` block at 16 x 16), joined as the hourglass joins them
(nearest upsampling and residual sums), with a max pool where the hourglass has its stride-2 BasicBlock and nothing where it has the
stride-1 ones.  The arbiter is the float64 oracle's BottleNeck (oracle/torch_ref.py) in the same arrangement; the rule is
tests/test_infer_fuse_bneck_gpu.py::_check_forms: fused at most 3x the unfused distance from float64, floor 1e-4 of the peak, argmax
equal except at near-ties, second run the same bits -- eval and deployed form, the BottleNeck pass alone and with all four passes."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from litehandnet_amd.engine import PlanModule
from litehandnet_amd.liteHandNet import BottleNeck
from litehandnet_amd.plan import BNECK, FINALIZE
from oracle import synth, torch_ref
from test_infer_fuse_bneck_gpu import SETTERS, _check_forms, _fwd

pytestmark = pytest.mark.gpu
WIDTH = 256


@pytest.fixture(autouse=True)
def _switches_back():
    yield
    for f in SETTERS:
        f(None)


def _blocks(bneck, reduction):
    pair = lambda: nn.Sequential(bneck(WIDTH, reduction), bneck(WIDTH, reduction))
    return nn.ModuleList([pair() for _ in range(3)]), nn.ModuleList([pair() for _ in range(3)]), bneck(WIDTH, 2)


class Hourglass256(PlanModule):
    def __init__(self, reduction):
        super().__init__()
        self.encoder, self.decoder, self.neck = _blocks(BottleNeck, reduction)

    def emit(self, pb, x, out=None):
        enc = [x]
        for pair in self.encoder:
            x = pb.maxpool(x)
            for b in pair:
                x = b.emit(pb, x)
            enc.append(x)
        for i, pair in enumerate(self.decoder):
            for b in pair:
                x = b.emit(pb, x)
            if i:
                x = pb.ew([x, enc[3 - i]])          # nearest upsample + add
        return self.neck.emit(pb, pb.ew([x, enc[0]]))

    def deploy_model(self):
        for m in self.modules():
            if hasattr(m, "switch_to_deploy"):
                m.switch_to_deploy()
        self.deploy = True
        self.__dict__.pop("_engine", None)


class Hourglass256Ref(nn.Module):
    def __init__(self, reduction):
        super().__init__()
        self.encoder, self.decoder, self.neck = _blocks(torch_ref.BottleNeck, reduction)

    def forward(self, x):
        enc = [x]
        for pair in self.encoder:
            x = pair(F.max_pool2d(x, 2, 2, ceil_mode=True))
            enc.append(x)
        for i, pair in enumerate(self.decoder):
            x = pair(x)
            if i:
                x = F.interpolate(x, size=enc[3 - i].shape[2:]) + enc[3 - i]
        return self.neck(F.interpolate(x, size=enc[0].shape[2:]) + enc[0])


def _pair256(reduction, seed):
    ref = Hourglass256Ref(reduction)
    sd = synth.synth_state_dict(ref, seed)
    ref.load_state_dict(sd)
    m = Hourglass256(reduction)
    m.load_state_dict(sd)
    return m, ref.double().eval()


def _input(seed):
    return torch.randn(2, WIDTH, 16, 16, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("reduction,mids", [(4, {(64, 8), (64, 4), (64, 2), (128, 16)}), (2, {(128, 16), (128, 8), (128, 4), (128, 2)})])
def test_width_256_eval_and_deployed(dev, reduction, mids):
    m, ref = _pair256(reduction, 29)
    m.to(dev).eval()
    x = _input(5)
    _, p = _fwd(m, x.to(dev), "bneck")
    fused = [r for r in p.pb.recs if r["op"] == BNECK]
    assert all(r["x"].C == WIDTH for r in fused) and {(r["mids"][0].C, r["x"].H) for r in fused} == mids
    assert sorted(r["x"].H for r in fused) == [2] * 6 + [4] * 4 + [8] * 2 + [16]
    _check_forms(f"hg256_r{reduction}", m, ref, x, dev, 13)


def test_tables_follow_the_parameters_256(dev):
    """The table cache at this width: after the 3x3 weights (the tap-major scratch holds a copy) and the BatchNorm behind t2 change,
    the next fused eval forward equals one from a freshly built plan."""
    m, _ = _pair256(4, 43)
    m.to(dev).eval()
    x = _input(7).to(dev)
    y1, p = _fwd(m, x, "bneck")
    assert torch.equal(y1, _fwd(m, x, "bneck")[0]) and p._table_sig is not None

    def fresh():
        m.__dict__.pop("_engine", None)
        return _fwd(m, x, "bneck")[0]
    for cm in (64, 128):
        rec = next(r for r in p.pb.recs if r["op"] == BNECK and r["mids"][0].C == cm)
        bn2 = next(r["bn"] for r in p.pb.recs if r["op"] == FINALIZE and r["out"].buf == rec["mids"][1].buf)     # the BatchNorm behind t2
        with torch.no_grad():
            bn2.bias.add_(0.5)
            bn2.running_var.mul_(2.0)
            rec["convs"][1].weight.mul_(1.5)
        y2, p = _fwd(m, x, "bneck")
        assert not torch.equal(y2, y1)
        assert torch.equal(y2, fresh())
        y1, p = _fwd(m, x, "bneck")
