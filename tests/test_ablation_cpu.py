"""CPU: the `hourglass_ablation` family -- registry, state_dict contract, initial state, the restatement against the reference's
recorded results, and the plans (built without a GPU, as tests/test_plan_cpu.py builds them)."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import ablation_ref
from litehandnet_amd import get_model
from litehandnet_amd.config import litehandnet_cfg
from litehandnet_amd.plan import ATT_MLP, CBAM, DWPW, KXK, PW, SE_MLP, PlanBuilder
from oracle import heatmap_np as onp
from oracle import synth, torch_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INIT = json.load(open(os.path.join(GOLD, "init_weights_ablation.json")))
TAGS = list(ablation_ref.TAGS)


def _cfg(tag, size=128, **kw):
    cfg = litehandnet_cfg("X", image_size=size, **dict(ablation_ref.TAGS[tag], **kw))
    cfg.MODEL["ca_dropout"] = 0.0
    return cfg


def _plan(model, n=2, size=128, backward=True, fuse=False):
    tensors = list(model.state_dict(keep_vars=True).values())
    pb = PlanBuilder(n, {id(t): j for j, t in enumerate(tensors)}, image_hw=(size, size), with_backward=backward, p_drop=0.0,
                     infer_fuse=fuse, infer_fuse_dwpw=fuse, infer_fuse_msrb=fuse)
    y = model.emit(pb, pb.image())
    assert y.buf == -2 and (y.C, y.H, y.W) == (21, size // 4, size // 4)
    return pb, pb.finalize()


def test_registry_returns_the_cbam_model():
    """The name `hourglass_ablation` used to end in get_model's assert."""
    m = get_model(litehandnet_cfg("X", ca_type="cbam"))
    assert type(m).__name__ == "hourglass_ablation"
    assert sum(p.numel() for p in m.parameters()) == ablation_ref.PARAMS["cbam"]


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_the_fixture(tag):
    """tests/ablation_ref.py in float32 on the CPU gives the reference's recorded heatmap, loss, gradient norms and running
    mean (the generator proved bit equality; another host's BLAS may round sums differently, hence tolerances)."""
    g = np.load(os.path.join(GOLD, f"model_X{tag}_128.npz"))
    cfg = _cfg(tag)
    n, size, seed = int(g["n"]), int(g["size"]), int(g["seed"])
    ref = ablation_ref.get_model(cfg, p_drop=0.0)
    ref.load_state_dict(synth.synth_state_dict(ref, seed))
    ref.train()
    j = synth.synth_joints(n, 21, size, seed + 1)
    tgt = np.stack([onp.msra_generate_target(a, np.ones_like(a), [size, size], [size // 4, size // 4])[0] for a in j])
    y = ref(synth.synth_images(n, size, seed))
    loss, _ = torch_ref.TopdownHeatmapLoss(cfg)(y, {"target": torch.from_numpy(tgt), "target_weight": torch.from_numpy(g["target_weight"])})
    loss.backward()
    assert np.abs(y.detach().numpy() - g["heatmap"]).max() <= 1e-4 * np.abs(g["heatmap"]).max()
    assert abs(float(loss.detach()) - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))
    gn = {k: float(p.grad.double().norm()) for k, p in ref.named_parameters()}
    assert sorted(gn) == g["grad_keys"].tolist()
    top = max(g["grad_norms"])
    for k, want in zip(g["grad_keys"].tolist(), g["grad_norms"].tolist()):
        assert abs(gn[k] - want) <= 2e-3 * (want + 1e-3 * top), (k, gn[k], want)
    assert np.allclose(ref.state_dict()[str(g["bn_key"])].numpy(), g["bn_running_mean"], rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("tag", TAGS)
def test_state_dict_contract(tag):
    g = np.load(os.path.join(GOLD, f"model_X{tag}_128.npz"))
    m = get_model(_cfg(tag))
    sd = m.state_dict()
    assert list(sd) == g["state_keys"].tolist()
    assert [",".join(map(str, v.shape)) for v in sd.values()] == g["state_shapes"].tolist()
    assert list(sd) == list(ablation_ref.get_model(_cfg(tag)).state_dict())
    assert sum(p.numel() for p in m.parameters()) == ablation_ref.PARAMS[tag]
    if tag == "cbam":
        att = [k for k in sd if k.startswith("hgs.encoder.0.att.")]
        assert len(att) == 19 and tuple(sd["hgs.encoder.0.att.sa.conv.weight"].shape) == (1, 2, 7, 7)
        assert tuple(sd["hgs.encoder.0.att.ca.sharedMLP.0.weight"].shape) == (8, 128, 1, 1)


@pytest.mark.parametrize("tag", TAGS)
def test_initial_state_equals_the_reference(tag):
    """init_weights (hourglass_ablation.py:305-311): convolutions ~ N(0, 1) with bias 0, BatchNorm 1 / 0, nn.Linear untouched --
    under the same torch seed the mirror and the restatement give the reference's bytes."""
    e = INIT["models"][tag]
    for build in (get_model, ablation_ref.get_model):
        torch.manual_seed(INIT["seed"])
        sd = build(litehandnet_cfg("X", **e["kw"])).state_dict()
        assert len(sd) == e["tensors"]
        for k, want in e["sums"].items():
            assert float(sd[k].double().sum()) == want, (tag, build.__module__, k)
        h = hashlib.sha256()
        for k, v in sd.items():
            h.update(k.encode())
            h.update(v.detach().cpu().contiguous().numpy().tobytes())
        assert h.hexdigest() == e["sha256"], (tag, build.__module__)
    if tag in ("se", "rca"):        # nn.Linear keeps torch's default: |w| <= 1 / sqrt(fan_in), never N(0, 1)
        lin = [m for m in get_model(litehandnet_cfg("X", **e["kw"])).modules() if isinstance(m, torch.nn.Linear)]
        assert lin and all(float(m.weight.abs().max()) <= 1.0 / m.in_features ** 0.5 + 1e-6 for m in lin)


def test_unknown_ca_type_and_block_counts_fail_as_the_reference_does():
    with pytest.raises(ValueError):
        get_model(litehandnet_cfg("X", ca_type="sk"))
    with pytest.raises(AssertionError):
        get_model(litehandnet_cfg("X", msrb=False, num_block=[2, 2, 2]))
    with pytest.raises(AssertionError):
        get_model(litehandnet_cfg("X", num_block=[2, 2, 2, 2]))
    # msrb=False never reads ca_type: configs _1_ (ca) and _7_ (identity) are one network
    a = get_model(litehandnet_cfg("X", msrb=False, num_block=[2, 2, 2, 2], ca_type="ca"))
    b = get_model(litehandnet_cfg("X", msrb=False, num_block=[2, 2, 2, 2], ca_type="identity"))
    assert [(k, tuple(v.shape)) for k, v in a.state_dict().items()] == [(k, tuple(v.shape)) for k, v in b.state_dict().items()]


@pytest.mark.parametrize("tag", TAGS + ["ca"])
def test_plans_build(tag):
    m = get_model(_cfg(tag) if tag != "ca" else litehandnet_cfg("X", image_size=128, ca_dropout=0.0))
    pb, (cb, cf, cbw, nf, nb) = _plan(m)
    assert nf >= len([r for r in pb.recs if not r.get("lazy")]) and nb > nf
    kinds = [r["op"] for r in pb.recs]
    want = {"nomsrb": (0, 0, 0), "se": (0, 2, 0), "1x1": (0, 0, 0), "id": (0, 0, 0), "cbam": (0, 0, 2), "rca": (8, 0, 0), "ca": (2, 0, 0)}[tag]
    assert (kinds.count(ATT_MLP), kinds.count(SE_MLP), kinds.count(CBAM)) == want
    if tag == "cbam":
        for r in (r for r in pb.recs if r["op"] == CBAM):
            prods = {id(q): q["op"] for q in pb.recs if q["op"] in (KXK, PW) and q["out"].buf in (r["p"].buf, r["r"].buf)}
            assert sorted(prods.values()) == sorted([KXK, PW])
            assert not pb.bufs[r["p"].buf].gate and not pb.bufs[r["out"].buf].gate and "scratch" in r
        # forward-only plans allocate no backward scratch
        pf, _ = _plan(m, backward=False)
        assert all("scratch" not in r for r in pf.recs if r["op"] == CBAM) and pf.ar["misc"].size < pb.ar["misc"].size


def test_rca_adds_six_attentions_to_the_ca_network():
    ca, _ = _plan(get_model(litehandnet_cfg("X", image_size=128, ca_dropout=0.0)))
    rca, _ = _plan(get_model(_cfg("rca")))
    n = lambda pb: sum(r["op"] == ATT_MLP for r in pb.recs)      # noqa: E731
    assert n(rca) == n(ca) + 6


@pytest.mark.parametrize("tag", TAGS)
def test_inference_fusion_switches_keep_working(tag):
    """All three switches on: the forward-only plan builds; fuse_dw_pw finds the 16 DWConv pairs it finds in mynet (none without
    ME_att), the other two passes find nothing to fuse in this family."""
    m = get_model(_cfg(tag)).eval()
    pb, (_, _, _, nf, nb) = _plan(m, backward=False, fuse=True)
    assert nb == 0 and nf > 0
    assert pb.n_fused_dwpw == (0 if tag == "nomsrb" else 16) == sum(r["op"] == DWPW for r in pb.recs)
    assert pb.n_fused == 0 and pb.n_fused_msrb == 0
    mm, _ = _plan(get_model(litehandnet_cfg("M", image_size=128, ca_dropout=0.0)).eval(), backward=False, fuse=True)
    assert tag == "nomsrb" or mm.n_fused_dwpw == pb.n_fused_dwpw
