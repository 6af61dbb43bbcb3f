"""GPU (MI355X): the lane-quad PCG kernel (mpcgpu_amd/csrc/pcg_lqb.hip.h, family 11) computes the SAME BITS as the commit recorded in
tests/golden/lqb_bits_parent.npz (tests/make_lqb_bits.py wrote it, on the GPU, on the parent of the change that gave the loop's stages
issue priorities; the hash is in the file).  A change of that loop may move instructions, addresses and issue order, never an operand, an
operation or an order of summation — so every output is compared with assert_array_equal: lambda, pcg_iters, pcg_exit of the batched solve at N = 128, 64, 32
and the ragged horizon 100, SS and block-Jacobi, exit_tol 0 at max_iter 1, 10, 167, one tolerance exit per preconditioner, and d_r / d_p
of the reference-style entry.
"""
import os

import numpy as np
import pytest

import make_lqb_bits as M

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
        S, Pinv, g, digest = M.inputs(N, pc)
        assert digest == str(rec[M.key(N, pc, "inputs_sha256")]), f"the seeded inputs of N={N} {pc} are not the recorded ones: nothing about the kernel can be concluded"
        _inputs[(N, pc)] = (S, Pinv, g)
    return _inputs[(N, pc)]


def test_record_is_small_and_names_its_commit(rec):
    assert os.path.getsize(M.OUT) < 700 * 1024
    assert len(str(rec["commit"])) == 40


@pytest.mark.parametrize("K", M.MAX_ITERS)
@pytest.mark.parametrize("pc", M.PRECONDS)
@pytest.mark.parametrize("N", M.HORIZONS)
def test_lqb_fixed_iterations_same_bits(gpu, rec, N, pc, K):
    S, Pinv, g = inputs(rec, N, pc)
    lam, it, ex = M.solve(N, pc, S, Pinv, g, K, 0.0)
    np.testing.assert_array_equal(it, rec[M.key(N, pc, f"K{K}_iters")])
    np.testing.assert_array_equal(ex, rec[M.key(N, pc, f"K{K}_exit")])
    np.testing.assert_array_equal(lam.view(np.uint32), rec[M.key(N, pc, f"K{K}_lambda")].view(np.uint32))


@pytest.mark.parametrize("N,pc", M.TOL_CASES)
def test_lqb_tolerance_exit_same_bits(gpu, rec, N, pc):
    S, Pinv, g = inputs(rec, N, pc)
    lam, it, ex = M.solve(N, pc, S, Pinv, g, 167, float(rec[M.key(N, pc, "tol")]))
    np.testing.assert_array_equal(it, rec[M.key(N, pc, "tol_iters")])
    np.testing.assert_array_equal(ex, rec[M.key(N, pc, "tol_exit")])
    assert (ex == 0).all() and (it < 167).all()
    np.testing.assert_array_equal(lam.view(np.uint32), rec[M.key(N, pc, "tol_lambda")].view(np.uint32))


def test_lqb_reference_entry_same_bits(gpu, rec):
    N, K = M.REF_CASE
    S, Pinv, g = inputs(rec, N, "ss")
    lam, r, p, it, ex = M.solve_ref(N, S, Pinv, g, K)
    np.testing.assert_array_equal(it, rec["ref_iters"])
    np.testing.assert_array_equal(ex, rec["ref_exit"])
    for got, name in ((lam, "ref_lambda"), (r, "ref_d_r"), (p, "ref_d_p")):
        np.testing.assert_array_equal(got.view(np.uint32), rec[name].view(np.uint32), err_msg=name)
