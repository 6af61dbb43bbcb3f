"""GPU (MI355X): the lane-quad PCG kernel (mpcgpu_amd/csrc/pcg_lqb.hip.h, family 11) computes the SAME BITS as the commit recorded in
tests/golden/lqb_bits_tail_parent.npz (tests/make_lqb_bits_tail.py wrote it, on the GPU, on the parent of the change that re-cut the tail of a
pass; the hash is in the file) on the paths tests/test_gpu_lqb_bits.py does not reach: a random lambda0 (the set-up S pass multiplies something),
batch 3, horizons that leave the last wavefront partly (100) or almost wholly (113, 17) empty — the masked publishing stores — and d_r / d_p of
the reference-style entry at an iteration-cap exit (p pending: the write-back forms it) and at a tolerance exit.  Every output is compared with
assert_array_equal on its bit pattern.
"""
import os

import numpy as np
import pytest

import make_lqb_bits_tail as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rec():
    d = np.load(M.OUT)
    return {k: d[k] for k in d.files}


@pytest.fixture(scope="module")
def gpu():
    import torch
    from mpcgpu_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()


_inputs = {}


def inputs(rec, N, pc):
    if (N, pc) not in _inputs:
        S, Pinv, g, lam0, digest = M.inputs(N, pc)
        assert digest == str(rec[M.key(N, pc, "inputs_sha256")]), f"the seeded inputs of N={N} {pc} are not the recorded ones: nothing about the kernel can be concluded"
        _inputs[(N, pc)] = (S, Pinv, g, lam0)
    return _inputs[(N, pc)]


def test_record_is_small_and_names_its_commit(rec):
    assert os.path.getsize(M.OUT) < 200 * 1024
    assert len(str(rec["commit"])) == 40


@pytest.mark.parametrize("N,pc,K", [(N, pc, K) for N, pc, caps in M.CASES for K in caps])
def test_lqb_tail_fixed_iterations_same_bits(gpu, rec, N, pc, K):
    S, Pinv, g, lam0 = inputs(rec, N, pc)
    lam, it, ex = M.solve(N, pc, S, Pinv, g, lam0, K, 0.0)
    np.testing.assert_array_equal(it, rec[M.key(N, pc, f"K{K}_iters")])
    np.testing.assert_array_equal(ex, rec[M.key(N, pc, f"K{K}_exit")])
    assert lam.shape == (M.BATCH, 14 * N)
    np.testing.assert_array_equal(lam.view(np.uint32), rec[M.key(N, pc, f"K{K}_lambda")].view(np.uint32))


def _check_ref(rec, prefix, res):
    for name, got in zip(M.REF_NAMES, res):
        want = rec[prefix + name]
        if got.dtype == np.float32:
            got, want = got.view(np.uint32), want.view(np.uint32)
        np.testing.assert_array_equal(got, want, err_msg=prefix + name)


def test_lqb_tail_reference_entry_cap_exit_same_bits(gpu, rec):
    S, Pinv, g, lam0 = inputs(rec, M.REF_N, "ss")
    res = M.solve_ref(M.REF_N, S, Pinv, g, lam0, M.REF_CAP, 0.0)
    assert res[3][0] == M.REF_CAP and res[4][0] == 1
    _check_ref(rec, "refcap_", res)


def test_lqb_tail_reference_entry_tolerance_exit_same_bits(gpu, rec):
    S, Pinv, g, lam0 = inputs(rec, M.REF_N, "ss")
    res = M.solve_ref(M.REF_N, S, Pinv, g, lam0, 167, float(rec["reftol_tol"]))
    assert res[4][0] == 0 and res[3][0] < 167
    _check_ref(rec, "reftol_", res)
