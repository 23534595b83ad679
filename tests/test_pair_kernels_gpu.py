"""The two-job entry points (lhn_maxpool2_fwd_pair, lhn_maxpool2_bwd_pair, lhn_ew_fwd_pair, lhn_ew_bwd_pair, lhn_ew_bwd_multi_pair,
lhn_avgpool_fwd_pair, lhn_bn_finalize_pair) against the two single calls they stand for: every case of tests/pair_cases.py runs the
pair entry once and the two single entries once on copies of the same inputs, and every buffer either may write -- y, dx, pooled means,
tables, running statistics, num_batches_tracked, mean | invstd, and every float around the views -- must be BIT-IDENTICAL.  The single
entries are the reference; tests/test_ew_pool_gpu.py and tests/test_bn_gpu.py hold them to float64.

BatchNorm-backward sums are added with atomics.  Under LHN_DETERMINISTIC=1 (a child process, as the other suites do) they must be
bit-identical too, because each job keeps its grid and its replicas.  In the default mode they are held to the bar of
tests/test_ew_pool_gpu.py against float64: max(2e-5, 3 x the float32 reference's own error), both taken over the sums of all replicas
and relative to the largest sum.

A pair entry refuses unequal geometry, overlapping outputs, a pool with statistics and a bilinear combine with the reason in
lhn_last_error(), and writes nothing."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pair_cases as pc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FLOOR = 2e-5        # the project's kernel-level floor (test_ew_pool_gpu.FLOOR)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.reshape(-1).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _compare(case, got, ref, sums_exact):
    assert got.keys() == ref.keys()
    for k in got:
        if k.startswith("ref.") or (k == pc.SUMS.get(case) and not sums_exact):
            continue
        np.testing.assert_array_equal(_bits(got[k]), _bits(ref[k]), err_msg=f"{case}: {k}")
    name = pc.SUMS.get(case)
    if name is None:
        return
    # the sums against float64, whatever the mode: the bar of tests/test_ew_pool_gpu.py
    r64, r32 = pc.sums_reference(ref, torch.float64), pc.sums_reference(ref, torch.float32)
    e32 = pc.rel_err(r32, r64)
    bar = max(FLOOR, 3 * e32)
    c = r64.shape[1]
    coff = int(ref["ref.coff"])
    for tag, out in (("pair", got), ("single", ref)):
        tot = out[name].sum(0)                                # over the replicas: [2][producer channels]
        err = pc.rel_err(tot[:, coff:coff + c], r64)
        same = np.array_equal(_bits(got[name]), _bits(ref[name]))
        print(f"pair {case} {name} ({tag}): err {err:.3e} e32 {e32:.3e} bar {bar:.3e} bit-equal to the single calls {same}")
        assert err <= bar, f"{case}: {name} of the {tag} form: err {err:.3e} > bar {bar:.3e}"
        outside = np.concatenate([tot[:, :coff].reshape(-1), tot[:, coff + c:].reshape(-1)])
        assert not outside.any(), f"{case}: {name}: sums outside the view's channels"
    assert float(np.abs(r64).max()) > 0


@pytest.mark.parametrize("case", pc.CASES)
def test_pair_entry_writes_the_bits_of_the_two_single_calls(dev, case):
    rc, got = pc.run(case, dev, True)
    assert rc == 0, pc._lib.lib().lhn_last_error().decode()
    rc, ref = pc.run(case, dev, False)
    assert rc == 0, pc._lib.lib().lhn_last_error().decode()
    assert any(not np.all(v == pc.PREFILL) for k, v in ref.items() if not k.startswith("ref."))       # something was written
    _compare(case, got, ref, sums_exact=False)


def test_finalize_pair_steps_each_num_batches_tracked_by_one(dev):
    _, got = pc.run("finalize_train", dev, True)
    assert int(got["nbt0"][0]) == 4 and int(got["nbt1"][0]) == 6
    _, got = pc.run("finalize_eval", dev, True)
    assert int(got["nbt0"][0]) == 3 and int(got["nbt1"][0]) == 5 and np.all(got["save0"] == pc.PREFILL)


def test_deterministic_mode_is_bit_identical_sums_included(dev, tmp_path):
    out = str(tmp_path / "pair.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "pair_cases.py"), out], env=dict(os.environ, LHN_DETERMINISTIC="1"),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = dict(np.load(out))
    for case in pc.CASES:
        got, ref = ({k[len(f"{case}/{p}/"):]: v for k, v in res.items() if k.startswith(f"{case}/{p}/")} for p in (1, 0))
        assert got
        _compare(case, got, ref, sums_exact=True)


@pytest.mark.parametrize("case", list(pc.REFUSE))
def test_pair_entry_refuses_and_writes_nothing(dev, case):
    rc, out = pc.run(case, dev, True)
    err = pc._lib.lib().lhn_last_error().decode()
    assert rc != 0 and pc.REFUSE[case] in err, f"{case}: status {rc}, error {err!r}"
    for k, v in out.items():
        assert np.all(v == pc.PREFILL), f"{case}: a refused call wrote to {k}"
    rc, _ = pc.run(case, dev, False)            # the same arguments as two single calls are served
    assert rc == 0, pc._lib.lib().lhn_last_error().decode()
