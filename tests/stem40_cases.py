"""Cases of the stem convolution with 40 output channels (3 -> 40, k = 3: my_pelee_stem.conv1 of mynet at width 160, 40 = 160 / 4), run
through the C ABI with the harness of tests/stem_cases.py: its runners, references and `*_ok` guards.  The cases are registered in
that module's lookup dictionary (`_ALL`) at import and nowhere else, so its own tables stay as they are.  Imported by
tests/test_stem40_gpu.py; as a script (a child process with its own environment):
    python tests/stem40_cases.py OUT.npz REPEATS fwd:NAME bwd:NAME ...
    python tests/stem40_cases.py --check-reference        (CPU only)

40 output channels run on the direct kernels k_stem_fwd / k_stem_bwd<3,3>: five groups of 8 channels give 51 pixel lanes per block
forward (thread 255 idle), ten groups of 4 give 25 pixel lanes backward (threads 250..255 idle).  An idle thread that took a pixel
would compute one that the next block owns as well: y would still be right, the statistics and dW would count it twice.  The
statistics of c40_concat and c40_s1 (more than 51 pixels) and dW of every case but c40_even (more than 25 pixels) would show it."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stem_cases as sc  # noqa: E402
from stem_cases import _case  # noqa: E402

CASES = {
    "c40_odd": sc._case(2, 9, 9, 3, 2, 1, 40, "fin ygate dpool"),                   # 5 x 5 outputs, 50 px; y = channels [8, 48) of 48
    "c40_even": sc._case(1, 8, 10, 3, 2, 1, 40, "fold"),                            # 4 x 5 outputs, 20 px: under one block's lanes
    "c40_concat": sc._case(2, 17, 19, 3, 2, 1, 40, "fin", yv=(96, 32)),             # 9 x 10 outputs, 180 px: several blocks; y inside a wider buffer
    "c40_whole": sc._case(2, 9, 9, 3, 2, 1, 40, yv=(40, 0)),                        # y is the whole buffer
    "c40_s1": sc._case(1, 9, 13, 3, 1, 1, 40, "fin"),                               # stride 1 of the same shape: 117 px
}
REFUSE = {"c24_again": _case(1, 9, 9, 3, 2, 1, 24, kind="fwd", refuse="Cout=24"),
          "c24_bwd": _case(1, 9, 9, 3, 2, 1, 24, kind="bwd", refuse="Cout=24"),
          "c40_k2": _case(1, 9, 9, 2, 1, 0, 40, kind="fwd", refuse="k=2")}
for _t in (CASES, REFUSE):
    for _k, _v in _t.items():
        assert _k not in sc._ALL, _k
        sc._ALL[_k] = _v


def _check_reference():
    for nm in CASES:
        g = sc.inputs(nm)
        assert g["seed"] == 7, f"{nm} needed seed {g['seed']}"
        assert sc.kernel_of(nm) == "k_stem_fwd" and sc.kernel_of(nm, kind="bwd") == "k_stem_bwd<3,3>"
        assert sc.direct_lds(CASES[nm]) <= sc.DIRECT_LDS_LIMIT
        for kind in ("fwd", "bwd"):
            r64, r32 = sc.reference(nm, g, kind=kind), sc.reference(nm, g, torch.float32, kind=kind)
            for k in r64:
                assert np.isfinite(r64[k]).all() and np.abs(r64[k]).max() > 0
                print(f"{kind}:{nm} {k}: e32 {sc.rel_err(r32[k], r64[k]):.2e}")


if __name__ == "__main__":
    if sys.argv[1] == "--check-reference":
        _check_reference()
        sys.exit(0)
    dst, reps, names = sys.argv[1], int(sys.argv[2]), sys.argv[3:]
    dev = torch.device("cuda:0")
    res = {}
    for full in names:
        kind, nm = full.split(":")
        g = sc.inputs(nm)
        for r in range(reps):
            for k, v in sc.run(nm, dev, g, kind=kind).items():
                res[f"{full}/{r}/{k}"] = v
    np.savez(dst, **res)
