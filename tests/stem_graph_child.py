"""Child of tests/test_infer_fuse_stem_gpu.py: variant A at 64 px in eval form with the stem fusion on, four forwards on a side stream
(LHN_GRAPH=1: the second one captures the launch sequence, the later ones replay it); saves the last output."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from litehandnet_amd import get_model, plan
from litehandnet_amd.config import litehandnet_cfg
from oracle import synth

cfg = litehandnet_cfg("A", image_size=64)
cfg.MODEL["ca_dropout"] = 0.0
m = get_model(cfg)
m.load_state_dict(synth.synth_state_dict(m, 3))
m.cuda().eval()
plan.set_infer_fuse_stem(True)
x = synth.synth_images(2, 64, 1).cuda()
side = torch.cuda.Stream()
side.wait_stream(torch.cuda.current_stream())
with torch.no_grad(), torch.cuda.stream(side):
    for it in range(4):
        y = m(x)
torch.cuda.synchronize()
p = next(iter(m.__dict__["_engine"].plans.values()))
assert p.pb.n_fused_stem == 1 and p.use_graph == (os.environ.get("LHN_GRAPH") == "1")
torch.save(y.cpu(), sys.argv[1])
print("CHECK", float(y.double().abs().sum()))
