"""The plan executor's switch LHN_PAIR_LAUNCH, end to end: one training step of MSRB(128) -> RepBasicUnit(128) on a 64 x 64 map and of
variant B on a 64 x 64 input, batch 2, under LHN_DETERMINISTIC=1, in two fresh child processes per model (tests/fwd_fin_child.py, the
method of tests/test_fwd_fin_step_gpu.py) -- the switch at 0 (every pool, combine and BatchNorm finalize a launch of its own) and at
its default (the two halves of a two-part tensor in one pool / combine launch, the two depthwise branches of an MSRB round in one
finalize launch).  Loss, output, every gradient and every BatchNorm buffer (running mean, running variance, num_batches_tracked) must
be bit-identical: a job of a pair launch keeps the grid, the replicas and the arithmetic of its single launch."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("which", ["block", "B"])
def test_train_step_is_bit_identical_with_and_without_the_switch(dev, tmp_path, which):
    res = []
    for mode in ("0", None):
        out = str(tmp_path / f"pair_{which}_{mode}.npz")
        env = {k: v for k, v in os.environ.items() if k != "LHN_PAIR_LAUNCH"}
        env["LHN_DETERMINISTIC"] = "1"
        if mode is not None:
            env["LHN_PAIR_LAUNCH"] = mode
        r = subprocess.run([sys.executable, os.path.join(HERE, "fwd_fin_child.py"), which, out], env=env, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        res.append(np.load(out))
    a, b = res
    assert set(a.files) == set(b.files) and any(k.startswith("g.") for k in a.files)
    assert any(k.startswith("b.") and k.endswith("running_mean") for k in a.files) and any(k.endswith("num_batches_tracked") for k in a.files)
    assert np.isfinite(a["loss"]) and float(np.abs(a["gflat"]).max()) > 0
    for k in a.files:
        x, y = a[k], b[k]
        u = {4: np.uint32, 8: np.uint64}[x.dtype.itemsize]
        np.testing.assert_array_equal(x.reshape(-1).view(u), y.reshape(-1).view(u), err_msg=k)
