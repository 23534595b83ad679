"""HIP-backed mirror of models/hourglass_ablation.py -- the registered `hourglass_ablation`, the network family behind the
paper's ablation table (config/hourglass_ablation/freihand/_1 ... _7_*.py).  It is `mynet` (pose_hg_ms_att.py) with three
constructor switches: `msrb` (ME_att against a plain Residual at the outermost level), `rca` (mynet's attention on every
Residual) and `ca_type` (what follows ME_att's second BRC: 'ca', 'se', '1x1', 'identity' or 'cbam').  Same class names,
constructor arguments, attribute names and Sequential indices as the reference, hence the same state_dict keys and OIHW
shapes.  DWConv, BottleNeck, BasicBlock, BRC and my_pelee_stem are the reference's text unchanged, so they are mynet's
classes; Residual, ME_att, EncoderDecoder and the model differ and are written here.

Five of the six distinct networks are assembled from the kernels of the other variants.  The sixth, ca_type='cbam', adds the
CBAM kernels of csrc/k_cbam.hip (PlanBuilder.cbam_attention)."""
from torch import nn

from .engine import PlanModule
from .pose_hg_ms_att import BRC, BasicBlock, BottleNeck, DWConv, _slope_of, my_pelee_stem

__all__ = ["DWConv", "BottleNeck", "BasicBlock", "BRC", "my_pelee_stem", "Residual", "ME_att", "EncoderDecoder", "CBAM",
           "hourglass_ablation"]


def _region_attention(out_c, p_drop):
    """mynet's attention Sequential (hourglass_ablation.py:73-82 and :191-200, the same text twice)."""
    return nn.Sequential(nn.AdaptiveAvgPool2d((3, 3)), nn.BatchNorm2d(out_c), nn.ReLU(),
                         nn.Conv2d(out_c, out_c, 3, 1, 0, groups=out_c), nn.Flatten(), nn.Dropout(p=p_drop),
                         nn.Linear(out_c, out_c), nn.Sigmoid())


class Residual(PlanModule):
    """hourglass_ablation.py:66-90: mynet's Residual, with `rca` its attention gates the output."""

    def __init__(self, inp_dim, out_dim, stride=1, num_block=2, rca=False, p_drop=0.3):
        super().__init__()
        self.conv1 = BasicBlock(inp_dim, out_dim, stride)
        self.blocks = nn.Sequential(*[BottleNeck(out_dim) for _ in range(num_block)])
        self.rca = rca
        if rca:
            self.att = _region_attention(out_dim, p_drop)

    def emit(self, pb, x, out=None):
        x = self.conv1.emit(pb, x)
        for b in self.blocks:
            x = b.emit(pb, x)
        return pb.me_attention(x, self.att) if self.rca else x      # (x is the whole plain buffer the last block wrote)


class RegionChannelAttention(nn.Module):
    """attention.py:234-250: parameters only (sharedMLP = 1x1 conv C -> C/r, ReLU, 1x1 conv C/r -> C, no biases)."""

    def __init__(self, in_planes, reduction=16):
        super().__init__()
        self.avg_pool, self.max_pool = nn.AdaptiveAvgPool2d(1), nn.AdaptiveMaxPool2d(1)
        self.sharedMLP = nn.Sequential(nn.Conv2d(in_planes, in_planes // reduction, 1, bias=False), nn.ReLU(),
                                       nn.Conv2d(in_planes // reduction, in_planes, 1, bias=False))
        self.sigmoid = nn.Sigmoid()


class RegionSpatialAttention(nn.Module):
    """attention.py:253-266: parameters only (a 7x7 convolution 2 -> 1 without bias)."""

    def __init__(self, kernel_size=7):
        super().__init__()
        assert kernel_size in (3, 7), "kernel size must be 3 or 7"
        self.conv = nn.Conv2d(2, 1, kernel_size, padding=(kernel_size - 1) // 2, bias=False)
        self.sigmoid = nn.Sigmoid()


class CBAM(PlanModule):
    """attention.py:269-294 (19 state_dict entries).  `pre` and `residual_conv` are the library's convolutions; everything between
    them and the final ReLU -- global mean and max pool, the shared MLP, the per-pixel 7x7 gate -- runs in csrc/k_cbam.hip."""
    expansion = 1

    def __init__(self, inplanes, planes, reduction=16):
        super().__init__()
        self.pre = nn.Sequential(nn.Conv2d(inplanes, planes, 3, 1, 1), nn.BatchNorm2d(planes), nn.ReLU(inplace=True),
                                 nn.Conv2d(planes, planes, 3, 1, 1), nn.BatchNorm2d(planes))
        self.residual_conv = nn.Conv2d(inplanes, planes, 1, 1)
        self.ca = RegionChannelAttention(planes, reduction)
        self.sa = RegionSpatialAttention()
        self.relu = nn.ReLU()

    def emit(self, pb, x, out=None):
        return pb.cbam_attention(x, self)


class ME_att(PlanModule):
    """hourglass_ablation.py:160-234: mynet's ME_att with a choice of what follows conv2."""

    def __init__(self, in_c, out_c, ca_type="ca", reduction=16, p_drop=0.3):
        super().__init__()
        m = in_c // 2
        self.conv1 = BRC(in_c, m, 1, 1, 0)
        self.mid1_conv = nn.ModuleList([nn.Sequential(DWConv(m, m // 2), DWConv(m // 2, m // 2)),
                                        nn.Sequential(DWConv(m, m), DWConv(m, m))])
        self.mid2_conv = nn.ModuleList([nn.Sequential(DWConv(m, m // 2, dilation=2, padding=2), DWConv(m // 2, m // 2)),
                                        nn.Sequential(DWConv(m, m, dilation=2, padding=2), DWConv(m, m))])
        self.conv2 = BRC(in_c, out_c, 1, 1, 0, bias=False)
        if ca_type == "ca":
            self.att = _region_attention(out_c, p_drop)
        elif ca_type == "se":
            self.att = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Flatten(), nn.Linear(out_c, out_c // reduction, bias=False),
                                     nn.ReLU(inplace=True), nn.Linear(out_c // reduction, out_c, bias=False), nn.Sigmoid())
        elif ca_type == "1x1":
            self.att = nn.Conv2d(out_c, out_c, 1, 1, 0)
        elif ca_type == "identity":
            self.att = nn.Identity()
        elif ca_type.lower() == "cbam":
            self.att = CBAM(out_c, out_c)
        else:
            raise ValueError(f"ERROR: {ca_type=}")
        self.ca_type = ca_type
        self.mid_c = m

    def emit(self, pb, x, out=None):
        m = self.conv1.emit(pb, x)
        for r in range(2):
            half = self.mid_c // 2 if r == 0 else self.mid_c
            cat = pb.new(m.H, m.W, 2 * half)
            for j, branch in enumerate((self.mid1_conv[r], self.mid2_conv[r])):
                branch[1].emit(pb, branch[0].emit(pb, m), out=pb.slice(cat, j * half, half))
            m = cat
        y = self.conv2.emit(pb, pb.ew([m, x]))
        if self.ca_type == "ca":
            return pb.me_attention(y, self.att)
        if self.ca_type == "se":
            # the two nn.Linear weights [J, C] / [C, J] are the 1x1 convolutions of an SEBlock without biases; the mean is
            # over the whole map whatever its shape (nn.AdaptiveAvgPool2d(1))
            return pb.se_attention(y, None, convs=(self.att[2], self.att[4]), global_pool=True)
        if self.ca_type == "1x1":
            return pb.conv(y, self.att, None)
        if self.ca_type == "identity":
            return y
        return self.att.emit(pb, y)


class EncoderDecoder(PlanModule):
    """hourglass_ablation.py:110-157.  msrb=False: Residuals at the outermost level too, one more num_blocks entry, and
    ca_type is never used."""

    def __init__(self, num_levels=5, inp_dim=128, num_blocks=[], msrb=True, rca=False, ca_type="ca", p_drop=0.3):
        super().__init__()
        self.num_levels = num_levels
        self.encoder, self.decoder = nn.ModuleList([]), nn.ModuleList([])

        def res(stride=1, nb=2):
            return Residual(inp_dim, inp_dim, stride, nb, rca=rca, p_drop=p_drop)

        if msrb:
            assert len(num_blocks) == num_levels - 1
            self.encoder.append(ME_att(inp_dim, inp_dim, ca_type, p_drop=p_drop))
            for i in range(num_levels - 1):
                self.encoder.append(res(2, num_blocks[i]))
                self.decoder.append(res())
            self.decoder.append(ME_att(inp_dim, inp_dim, ca_type, p_drop=p_drop))
        else:
            assert len(num_blocks) == num_levels
            self.encoder.append(res(1, num_blocks[0]))
            for i in range(num_levels - 1):
                self.encoder.append(res(2, num_blocks[i + 1]))
                self.decoder.append(res())
            self.decoder.append(res())

    def emit(self, pb, x, out=None):
        enc = []
        for layer in self.encoder:
            x = layer.emit(pb, x)
            enc.append(x)
        short = pb.avgpool(enc[0], enc[-1].H, enc[-1].W)
        for i, layer in enumerate(self.decoder):
            peer = enc[self.num_levels - 1 - i]
            x = pb.ew([layer.emit(pb, peer if i == 0 else x), short if i == 0 else peer])   # (+ nearest upsample)
        return x


class hourglass_ablation(PlanModule):
    """hourglass_ablation.py:272-311.  cfg.MODEL keys: num_stage, input_channel, output_channel, num_block, msrb, rca, ca_type
    (and mynet's ca_dropout for the 'ca' attention's nn.Dropout)."""
    consumes_image = True

    def __init__(self, cfg):
        super().__init__()
        M = cfg.MODEL
        num_stage = M.get("num_stage", 4)
        inp_dim = M.get("input_channel", 128)
        oup_dim = M.get("output_channel", cfg.DATASET.num_joints)
        num_block = M.get("num_block", [2, 2, 2])
        msrb = M.get("msrb", True)
        rca = M.get("rca", False)
        ca_type = M.get("ca_type", "ca")
        self.p_drop = float(M.get("ca_dropout", 0.3))
        self.pre = my_pelee_stem(inp_dim)
        self.hgs = EncoderDecoder(num_stage, inp_dim, num_block, msrb, rca, ca_type, p_drop=self.p_drop)
        self.features = nn.Sequential(BottleNeck(inp_dim), nn.Conv2d(inp_dim, inp_dim, 1, 1, 0), nn.BatchNorm2d(inp_dim),
                                      nn.LeakyReLU())
        self.outs = nn.Conv2d(inp_dim, oup_dim, 1, 1, 0)
        self.init_weights()

    def emit(self, pb, x, out=None):
        y = self.hgs.emit(pb, self.pre.emit(pb, x))
        y = self.features[0].emit(pb, y)
        y = pb.conv(y, self.features[1], self.features[2], slope=_slope_of(self.features[3]))
        return pb.conv(y, self.outs, None, nchw_out=True)

    def init_weights(self):
        # hourglass_ablation.py:305-311: conv weight ~ N(0,1), bias 0 (weight_init.py:28-32); BatchNorm gamma 1, beta 0;
        # nn.Linear keeps torch's default initialisation
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, 0, 1)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, (nn.BatchNorm2d, nn.GroupNorm)):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
