"""GPU: the full inverse from the kept upper dense factor (spp_dense_potri.h) through spp_dense_potri -- A is factored as
spp_dense_potrf_upper factors it, then Z = A^-1 is formed block row by block row, three launches each.

Matrices and the floor of the bound as in tests/test_gpu_dense_trsm.py (M M^T / n + 2 I, condition below 4, TOL 1e-11).
Per column j, the residual ||A z_j - e_j|| and the error ||z_j - numpy's|| / ||numpy's|| must be <= max(TOL, 4 x the same
quantity of spp_dense_posv_multi on the identity's columns). Z lies inside a NaN frame that must come back untouched; Z is
exactly symmetric; A comes back with the bits spp_dense_potrf_upper alone leaves; two runs agree bit for bit."""
import numpy as np
import pytest

from slam_plus_plus_amd import api
from test_gpu_dense_trsm import TOL, _spd, _potrf_alone, _posv_multi

pytestmark = pytest.mark.gpu

SHAPES = [1, 16, 17, 127, 128, 129, 300, 644, 1920, 2000]   # 1920: fifteen full tiles under ld = 2048
_CACHE = {}


def _matrix(n):
    """(A, numpy's inverse), computed once per shape"""
    if n not in _CACHE:
        A = _spd(n, 300 + n)
        _CACHE[n] = (A, np.linalg.inv(A))
    return _CACHE[n]


def _potri(ctx, A, ldz, frame=3):
    """returns (status, the whole Z buffer as (ldz, n + frame), the A buffer as (n, n))"""
    n = A.shape[0]
    dA = api.DeviceArray.from_host(ctx, np.asfortranarray(A).ravel(order="F"))
    dZ = api.DeviceArray.from_host(ctx, np.full(ldz * (n + frame), np.nan))
    st = ctx.dense_potri(dA.ptr, n, n, dZ.ptr, ldz)
    out = dZ.download().reshape((ldz, n + frame), order="F")
    R = dA.download().reshape((n, n), order="F")
    dA.free(); dZ.free()
    return st, out, R


def _figures(A, Zref, Z):
    n = A.shape[0]
    res = np.linalg.norm(A @ Z - np.eye(n), axis=0)
    err = np.linalg.norm(Z - Zref, axis=0) / np.linalg.norm(Zref, axis=0)
    return res, err


@pytest.mark.parametrize("n", SHAPES)
def test_potri_matches_numpy_and_touches_nothing_else(hip_ctx, n):
    A, Zref = _matrix(n)
    ldz = n if n == 128 else n + 5   # ldz = n once
    st, out, R = _potri(hip_ctx, A, ldz)
    assert st == 0
    Z = out[:n, :n]
    assert np.all(np.isnan(out[n:, :])) and np.all(np.isnan(out[:, n:])), "Z was written outside its n x n"
    assert not np.any(np.isnan(Z)), "Z was not written everywhere"
    assert np.array_equal(Z, Z.T), "Z is not exactly symmetric"
    st, base, _ = _posv_multi(hip_ctx, A, np.eye(n), n, extra_cols=0)   # the solve route on the identity's columns
    assert st == 0
    res, err = _figures(A, Zref, Z)
    res_b, err_b = _figures(A, Zref, base[:n, :n])
    print("n %d: largest residual %.3e (solve route %.3e), largest column error %.3e (solve route %.3e), floor %.0e" % (
        n, res.max(), res_b.max(), err.max(), err_b.max(), TOL))
    assert np.all(res <= np.maximum(TOL, 4.0 * res_b)), res
    assert np.all(err <= np.maximum(TOL, 4.0 * err_b)), err
    assert np.array_equal(R, _potrf_alone(hip_ctx, A)), "A differs from what spp_dense_potrf_upper alone leaves"
    _, again, _ = _potri(hip_ctx, A, ldz)
    assert np.array_equal(again[:n, :n], Z), "two runs differ"


def test_not_positive_definite_is_reported_and_leaves_Z(hip_ctx):
    n = 200
    A = _spd(n, 5)
    A[150, 150] = -1.0
    st, out, _ = _potri(hip_ctx, A, n + 5)
    assert st == api.SPP_NOT_POSDEF
    assert np.all(np.isnan(out)), "Z was written after a failed pivot"
    # and the ctx goes on working
    A2, Zref = _matrix(129)
    st, out, _ = _potri(hip_ctx, A2, 129 + 5)
    assert st == 0
    assert np.all(_figures(A2, Zref, out[:129, :129])[1] < TOL)


def test_bad_arguments(hip_ctx):
    A, _ = _matrix(127)
    dA = api.DeviceArray.from_host(hip_ctx, np.asfortranarray(A).ravel(order="F"))
    dZ = api.DeviceArray.from_host(hip_ctx, np.full(127 * 127, np.nan))
    lib, h = hip_ctx.lib, hip_ctx.h
    assert lib.spp_dense_potri(h, dA.ptr, 127, 127, dZ.ptr, 126) == -1   # ldz < n
    assert lib.spp_dense_potri(h, dA.ptr, 127, 126, dZ.ptr, 127) == -1   # ld < n
    assert lib.spp_dense_potri(h, dA.ptr, 0, 127, dZ.ptr, 127) == -1     # n < 1
    assert lib.spp_dense_potri(h, dA.ptr, 127, 127, None, 127) == -1
    assert lib.spp_dense_potri(h, None, 127, 127, dZ.ptr, 127) == -1
    assert lib.spp_dense_potri(None, dA.ptr, 127, 127, dZ.ptr, 127) == -1
    assert np.all(np.isnan(dZ.download())), "a refused call wrote Z"
    dA.free(); dZ.free()
