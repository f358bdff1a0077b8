"""GPU: the multi-column triangular solves on the upper dense factor (spp_dense_trsm.h) through spp_dense_posv_multi --
A is factored as spp_dense_potrf_upper factors it, then R^T R X = B runs a launch per block row and direction.

Systems as in tests/test_gpu_dense.py (M M^T / n + 2 I, condition below 4) and its bound for spp_dense_posv on them:
||x - numpy.linalg.solve|| / ||.|| < 1e-11 per column. B is asymmetric random; its rows >= n and columns >= k are NaN and
must come back untouched; A comes back with the bits spp_dense_potrf_upper alone leaves."""
import numpy as np
import pytest

from slam_plus_plus_amd import api

pytestmark = pytest.mark.gpu

TOL = 1e-11   # tests/test_gpu_dense.py::test_posv_matches_numpy
SHAPES = [(1, 1), (127, 15), (128, 16), (129, 17), (300, 1), (300, 129), (1920, 128), (2000, 33)]
_CACHE = {}


def _spd(n, seed):
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((n, n))
    return M @ M.T / n + np.eye(n) * 2.0


def _system(n, k):
    """(A, B, numpy's X), computed once per shape"""
    if (n, k) not in _CACHE:
        A = _spd(n, 300 + n)
        B = np.random.default_rng(7 * n + k).standard_normal((n, k))
        _CACHE[(n, k)] = (A, B, np.linalg.solve(A, B))
    return _CACHE[(n, k)]


def _posv_multi(ctx, A, B, ldb, extra_cols=2):
    """returns (status, the whole B buffer as (ldb, k + extra_cols), the A buffer as (n, n))"""
    n, k = B.shape
    buf = np.full((ldb, k + extra_cols), np.nan, order="F")
    buf[:n, :k] = B
    dA = api.DeviceArray.from_host(ctx, np.asfortranarray(A).ravel(order="F"))
    dB = api.DeviceArray.from_host(ctx, buf.ravel(order="F"))
    st = ctx.dense_posv_multi(dA.ptr, n, n, dB.ptr, ldb, k)
    out = dB.download().reshape((ldb, k + extra_cols), order="F")
    R = dA.download().reshape((n, n), order="F")
    dA.free(); dB.free()
    return st, out, R


def _potrf_alone(ctx, A):
    n = A.shape[0]
    dA = api.DeviceArray.from_host(ctx, np.asfortranarray(A).ravel(order="F"))
    assert ctx._check(ctx.lib.spp_dense_potrf_upper(ctx.h, dA.ptr, n, n)) == 0
    R = dA.download().reshape((n, n), order="F")
    dA.free()
    return R


@pytest.mark.parametrize("n,k", SHAPES)
def test_posv_multi_matches_numpy_and_touches_nothing_else(hip_ctx, n, k):
    A, B, Xr = _system(n, k)
    ldb = n if (n, k) == (128, 16) else n + 5   # ldb = n once
    st, out, R = _posv_multi(hip_ctx, A, B, ldb)
    assert st == 0
    X = out[:n, :k]
    err = np.linalg.norm(X - Xr, axis=0) / np.linalg.norm(Xr, axis=0)
    print("n %d k %d: largest column error %.3e (bound %.0e)" % (n, k, err.max(), TOL))
    assert np.all(err < TOL), err
    assert np.all(np.isnan(out[n:, :])) and np.all(np.isnan(out[:, k:])), "B was written outside its n rows / k columns"
    assert np.array_equal(R, _potrf_alone(hip_ctx, A)), "A differs from what spp_dense_potrf_upper alone leaves"


def test_a_column_has_the_bits_of_that_column_solved_alone(hip_ctx):
    """(300, 129): two passes; column j alone (k = 1, position 0) for a first, a last-of-tile, a first-of-next-tile, the
    last column of the first pass and the one column of the second; and two runs of the whole solve agree bit for bit"""
    n, k = 300, 129
    A, B, _ = _system(n, k)
    _, out, _ = _posv_multi(hip_ctx, A, B, n + 5)
    _, again, _ = _posv_multi(hip_ctx, A, B, n + 5)
    assert np.array_equal(out[:n, :k], again[:n, :k]), "two runs differ"
    for j in (0, 15, 16, 127, 128):
        _, one, _ = _posv_multi(hip_ctx, A, B[:, j:j + 1], n)
        assert np.array_equal(one[:n, 0], out[:n, j]), "column %d depends on its neighbours or its position" % j


def test_not_positive_definite_is_reported_and_leaves_B(hip_ctx):
    n, k = 200, 3
    A = _spd(n, 5)
    A[150, 150] = -1.0
    B = np.random.default_rng(1).standard_normal((n, k))
    st, out, _ = _posv_multi(hip_ctx, A, B, n + 5)
    assert st == api.SPP_NOT_POSDEF
    assert np.array_equal(out[:n, :k], B)
    # and the ctx goes on working
    A2, B2, Xr = _system(129, 17)
    st, out, _ = _posv_multi(hip_ctx, A2, B2, 129 + 5)
    assert st == 0 and np.all(np.linalg.norm(out[:129, :17] - Xr, axis=0) / np.linalg.norm(Xr, axis=0) < TOL)


def test_bad_arguments(hip_ctx):
    A, B, _ = _system(127, 15)
    dA = api.DeviceArray.from_host(hip_ctx, np.asfortranarray(A).ravel(order="F"))
    dB = api.DeviceArray.from_host(hip_ctx, np.asfortranarray(B).ravel(order="F"))
    lib, h = hip_ctx.lib, hip_ctx.h
    assert lib.spp_dense_posv_multi(h, dA.ptr, 127, 127, dB.ptr, 126, 15) == -1   # ldb < n
    assert lib.spp_dense_posv_multi(h, dA.ptr, 127, 127, dB.ptr, 127, 0) == -1    # nrhs < 1
    assert lib.spp_dense_posv_multi(h, dA.ptr, 127, 127, None, 127, 15) == -1
    assert lib.spp_dense_posv_multi(h, None, 127, 127, dB.ptr, 127, 15) == -1
    dA.free(); dB.free()
