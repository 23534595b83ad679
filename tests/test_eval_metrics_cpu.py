"""CPU: the dataset-level evaluation entry points exist in the C ABI (header, symbol list, library), the state size follows the
layout documented in include/lhn.h, and the evaluator has no host fallback."""
import os
import re

import numpy as np
import pytest
import torch

from litehandnet_amd import _lib, build
from litehandnet_amd.config import litehandnet_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lhn_eval_state_bytes", "lhn_eval_accumulate", "lhn_eval_finalize")


def test_symbols_declared_listed_exported():
    hdr = open(os.path.join(ROOT, "include", "lhn.h")).read()
    declared = set(re.findall(r"\b(lhn_[a-z0-9_]+)\s*\(", hdr))
    build.build_lib(verbose=False)
    L = _lib.lib()
    for s in NEW:
        assert s in declared and s in _lib.SYMBOLS and hasattr(L, s), s
    assert L.lhn_version() == 3
    for word in ("valid_pck", "hit_pck", "valid_auc", "hit_auc", "epe_cnt", "epe_hi", "epe_lo", "epe_bad"):
        assert word in hdr, word                      # the state layout is documented where the entry points are


def test_state_bytes_without_a_gpu():
    """valid_pck[K] | hit_pck[K] | valid_auc[K] | hit_auc[num_step][K] | epe_cnt, epe_hi, epe_lo, epe_bad: int64 words."""
    L = _lib.lib()
    for K, S in ((21, 20), (17, 20), (21, 1), (133, 20), (1, 1)):
        assert L.lhn_eval_state_bytes(K, S) == 8 * (3 * K + S * K + 4), (K, S)
    assert L.lhn_eval_state_bytes(0, 20) == 0 and L.lhn_eval_state_bytes(21, 0) == 0
    assert L.lhn_eval_state_bytes(1024, 20) == 0      # beyond the workgroup's counter space: refused, not truncated


def test_exports_and_signatures():
    import inspect

    import litehandnet_amd
    from litehandnet_amd import heatmap
    assert litehandnet_amd.TopDownEvaluator is heatmap.TopDownEvaluator
    assert litehandnet_amd.keypoint_auc is heatmap.keypoint_auc and litehandnet_amd.keypoint_epe is heatmap.keypoint_epe
    assert list(inspect.signature(heatmap.keypoint_auc).parameters) == ["pred", "gt", "mask", "normalize", "num_step"]
    assert inspect.signature(heatmap.keypoint_auc).parameters["num_step"].default == 20
    assert list(inspect.signature(heatmap.keypoint_epe).parameters) == ["pred", "gt", "mask"]
    p = inspect.signature(heatmap.TopDownEvaluator.__init__).parameters
    assert [p[k].default for k in ("metrics", "pck_thr", "auc_nor", "num_step")] == [("PCK", "AUC", "EPE"), 0.2, 30, 20]
    with pytest.raises(_lib.LhnError):
        heatmap.TopDownEvaluator(litehandnet_cfg("B"), metrics=["PCKh"])


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the behaviour of a GPU-less host")
def test_evaluator_refuses_to_run_without_a_gpu():
    from litehandnet_amd import heatmap
    p = np.zeros((2, 21, 2), np.float32)
    m = np.ones((2, 21), bool)
    ev = heatmap.TopDownEvaluator(litehandnet_cfg("B"))
    with pytest.raises(_lib.LhnError):
        ev.update_preds(p, p, m, np.ones(2, np.float32))
    meta = dict(center=np.zeros((2, 2), np.float32), scale=np.ones((2, 2), np.float32), joints_3d=np.zeros((2, 21, 3), np.float32),
                joints_3d_visible=np.ones((2, 21, 3), np.float32), bbox=np.ones((2, 4), np.float32))
    with pytest.raises(_lib.LhnError):
        ev.update(meta, torch.zeros(2, 21, 16, 16))
    for f in (lambda: heatmap.keypoint_auc(p, p, m, 30), lambda: heatmap.keypoint_epe(p, p, m), ev.compute, ev.state,
              ev.per_joint_pck):
        with pytest.raises(_lib.LhnError):
            f()
