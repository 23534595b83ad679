"""Plain-torch CPU restatement of the reference's `hourglass_ablation` (models/hourglass_ablation.py) -- the yardstick of
tests/test_ablation_cpu.py and tests/test_ablation_gpu.py.  oracle/torch_ref.py already restates `mynet`, whose DWConv,
BottleNeck, BasicBlock, BRC and stem the ablation file repeats word for word; those are reused and only what differs is
written here, from reading the reference, with its file:line next to every class.  Attribute names and Sequential indices
follow the reference's state_dict.  get_model(cfg, dtype=torch.float64) gives the float64 network.

tests/golden/make_golden_ablation.py proves it against the real reference bit for bit."""
import torch
from torch import nn
import torch.nn.functional as F

from oracle import torch_ref as T


def region_attention(c, p_drop):
    """hourglass_ablation.py:73-82 / :191-200: pool to 3x3 bins, BN, ReLU, depthwise 3x3 (valid), dropout, Linear, sigmoid."""
    return nn.Sequential(nn.AdaptiveAvgPool2d((3, 3)), nn.BatchNorm2d(c), nn.ReLU(), nn.Conv2d(c, c, 3, 1, 0, groups=c),
                         nn.Flatten(), nn.Dropout(p=p_drop), nn.Linear(c, c), nn.Sigmoid())


class Residual(nn.Module):
    """:66-90."""

    def __init__(self, cin, cout, stride=1, num_block=2, rca=False, p_drop=0.3):
        super().__init__()
        self.conv1 = T.MyBasicBlock(cin, cout, stride)
        self.blocks = nn.Sequential(*[T.MyBottleNeck(cout) for _ in range(num_block)])
        self.rca = rca
        if rca:
            self.att = region_attention(cout, p_drop)

    def forward(self, x):
        y = self.blocks(self.conv1(x))
        return y * self.att(y)[:, :, None, None] if self.rca else y


class ChannelGate(nn.Module):
    """attention.py:234-250: sigmoid(mlp(global mean) + mlp(global max)), one bias-free MLP of 1x1 convolutions for both."""

    def __init__(self, c, reduction=16):
        super().__init__()
        self.sharedMLP = nn.Sequential(nn.Conv2d(c, c // reduction, 1, bias=False), nn.ReLU(),
                                       nn.Conv2d(c // reduction, c, 1, bias=False))

    def forward(self, x):
        return torch.sigmoid(self.sharedMLP(F.adaptive_avg_pool2d(x, 1)) + self.sharedMLP(F.adaptive_max_pool2d(x, 1)))


class PixelGate(nn.Module):
    """attention.py:253-266: sigmoid(conv7x7([mean over channels, max over channels])), zero padding 3, no bias."""

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(2, 1, 7, padding=3, bias=False)

    def forward(self, x):
        s = torch.cat([x.mean(dim=1, keepdim=True), x.max(dim=1, keepdim=True)[0]], dim=1)
        return torch.sigmoid(self.conv(s))


class CBAM(nn.Module):
    """attention.py:269-294."""

    def __init__(self, cin, cout, reduction=16):
        super().__init__()
        self.pre = nn.Sequential(nn.Conv2d(cin, cout, 3, 1, 1), nn.BatchNorm2d(cout), nn.ReLU(),
                                 nn.Conv2d(cout, cout, 3, 1, 1), nn.BatchNorm2d(cout))
        self.residual_conv = nn.Conv2d(cin, cout, 1, 1)
        self.ca = ChannelGate(cout, reduction)
        self.sa = PixelGate()

    def forward(self, x):
        p = self.pre(x)
        u = self.ca(p) * p
        u = self.sa(u) * u
        return F.relu(u + self.residual_conv(x))


class ME_att(nn.Module):
    """:160-234."""

    def __init__(self, cin, cout, ca_type="ca", reduction=16, p_drop=0.3):
        super().__init__()
        m = cin // 2
        self.conv1 = T.BRC(cin, m, 1, 1, 0)
        self.mid1_conv = nn.ModuleList([nn.Sequential(T.MyDWConv(m, m // 2), T.MyDWConv(m // 2, m // 2)),
                                        nn.Sequential(T.MyDWConv(m, m), T.MyDWConv(m, m))])
        self.mid2_conv = nn.ModuleList([nn.Sequential(T.MyDWConv(m, m // 2, 2, 2), T.MyDWConv(m // 2, m // 2)),
                                        nn.Sequential(T.MyDWConv(m, m, 2, 2), T.MyDWConv(m, m))])
        self.conv2 = T.BRC(cin, cout, 1, 1, 0)
        if ca_type == "ca":
            self.att = region_attention(cout, p_drop)
        elif ca_type == "se":
            self.att = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Flatten(), nn.Linear(cout, cout // reduction, bias=False), nn.ReLU(),
                                     nn.Linear(cout // reduction, cout, bias=False), nn.Sigmoid())
        elif ca_type == "1x1":
            self.att = nn.Conv2d(cout, cout, 1, 1, 0)
        elif ca_type == "identity":
            self.att = nn.Identity()
        elif ca_type.lower() == "cbam":
            self.att = CBAM(cout, cout)
        else:
            raise ValueError(f"ERROR: {ca_type=}")
        self.gates = ca_type in ("se", "ca")

    def forward(self, x):
        t = self.conv1(x)
        for r in range(2):
            t = torch.cat([self.mid1_conv[r](t), self.mid2_conv[r](t)], dim=1)
        y = self.conv2(t + x)
        return y * self.att(y)[:, :, None, None] if self.gates else self.att(y)


class EncoderDecoder(nn.Module):
    """:110-157 (the data flow is variant A's hourglass)."""

    def __init__(self, levels, c, blocks, msrb=True, rca=False, ca_type="ca", p_drop=0.3):
        super().__init__()
        self.num_levels = levels
        self.encoder, self.decoder = nn.ModuleList(), nn.ModuleList()
        blocks = list(blocks)
        if msrb:
            assert len(blocks) == levels - 1
            self.encoder.append(ME_att(c, c, ca_type, p_drop=p_drop))
        else:
            assert len(blocks) == levels
            self.encoder.append(Residual(c, c, 1, blocks.pop(0), rca, p_drop))
        for nb in blocks:
            self.encoder.append(Residual(c, c, 2, nb, rca, p_drop))
            self.decoder.append(Residual(c, c, rca=rca, p_drop=p_drop))
        self.decoder.append(ME_att(c, c, ca_type, p_drop=p_drop) if msrb else Residual(c, c, rca=rca, p_drop=p_drop))

    forward = T._HourglassA.forward


class HourglassAblation(nn.Module):
    """:272-311.  cfg keys: MODEL.{num_stage,input_channel,output_channel,num_block,msrb,rca,ca_type}."""

    def __init__(self, cfg, p_drop=0.3):
        super().__init__()
        M = cfg.MODEL
        c = M.get("input_channel", 128)
        self.pre = T._StemM(c)
        self.hgs = EncoderDecoder(M.get("num_stage", 4), c, M.get("num_block", [2, 2, 2]), M.get("msrb", True),
                                  M.get("rca", False), M.get("ca_type", "ca"), p_drop)
        self.features = nn.Sequential(T.MyBottleNeck(c), *T._cbr(c, c, 1, act=nn.LeakyReLU()))
        self.outs = nn.Conv2d(c, M.get("output_channel", cfg.DATASET.num_joints), 1)
        self.init_weights()

    def forward(self, x):
        return self.outs(self.features(self.hgs(self.pre(x))[-1]))

    init_weights = T.MultiScaleAttentionHourglass.init_weights     # :305-311, the same rule: convolutions and BatchNorms only


def get_model(cfg, p_drop=0.3, dtype=torch.float32):
    assert cfg.MODEL.name == "hourglass_ablation"
    return HourglassAblation(cfg, p_drop).to(dtype)


# the six fixture networks (tests/golden/model_X<tag>_128.npz): tag -> litehandnet_cfg("X", **kw)
TAGS = {
    "nomsrb": dict(msrb=False, num_block=[2, 2, 2, 2]),      # configs _1_ and _7_: without ME_att, ca_type is never read
    "se": dict(ca_type="se"),
    "1x1": dict(ca_type="1x1"),
    "id": dict(ca_type="identity"),
    "cbam": dict(ca_type="cbam"),
    "rca": dict(rca=True),
}
PARAMS = {"nomsrb": 2760981, "se": 2208405, "1x1": 2237333, "id": 2204309, "cbam": 2832985, "rca": 2348693}
