"""GPU: spp_solve_device -- k further right-hand sides against the factor a dense Schur solve left behind
(spp_solve_again.hip on top of spp_dense_trsm.h).

Per fixture: spp_factor_solve_device with eta, then spp_solve_device on B = [eta, random, e of a camera row, e of a
landmark row, random ...]. Every column is held to
  - the residual ||Lambda x - b|| / ||b|| < 1e-11 (schur_ref.check_solution's bound on these fixtures), and
  - tests/parity.py's criterion with the EXISTING path as the reference backend: error against the refined solution
    <= max(1e-10, 4 x the error of spp_factor_solve_device on the same column, measured the same way).
The library's own new code is never the yardstick. The reference machinery (tests/solve_again_ref.py) is checked on the
host by tests/test_solve_again_ref_host.py, which also asserts cond(Lambda) < 1e6 for every fixture used here."""
import ctypes

import numpy as np
import pytest

import solve_again_ref as sar
from slam_plus_plus_amd import api

pytestmark = pytest.mark.gpu

RES_TOL = 1e-11
E_BADARG, E_STATE, E_UNSUPPORTED = -1, -5, -6
CASES = [(name, k) for name in sar.FIXTURES for k in (1, 6, 17)] + [("edges32", 129)]
_BASE = {}


def _open(name, mode=api.MODE_SCHUR):
    lam, eta = sar.problem(name)
    c = api.Context(0)
    c.analyze(lam, mode)
    dv = api.DeviceArray.from_host(c, lam.vals)
    return c, lam, eta, dv


def _factor(c, dv, eta):
    dr = api.DeviceArray.from_host(c, eta)
    st = c.factor_solve_device(dv.ptr, dr.ptr)
    x = dr.download()
    dr.free()
    return st, x


def _solve(c, dv, B, ldb=None, extra_cols=1):
    """spp_solve_device on a NaN-framed copy of B; returns the n x k result after checking the frame"""
    n, k = B.shape
    ldb = n + 3 if ldb is None else ldb
    buf = np.full((ldb, k + extra_cols), np.nan, order="F")
    buf[:n, :k] = B
    dB = api.DeviceArray.from_host(c, buf.ravel(order="F"))
    assert c.solve_device(dv.ptr, dB.ptr, k, ldb) == 0
    out = dB.download().reshape((ldb, k + extra_cols), order="F")   # (the download is ordered behind the solve)
    dB.free()
    assert np.all(np.isnan(out[n:, :])) and np.all(np.isnan(out[:, k:])), "B was written outside its n rows / k columns"
    return out[:n, :k]


def _baseline_err(name, c, dv):
    """error of the existing path on every column of the fixture's B against the refined solution, once per fixture"""
    if name not in _BASE:
        _BASE[name] = sar.col_err(sar.baseline_columns(c, dv.ptr, sar.rhs_columns(name)), sar.rhs_reference(name))
    return _BASE[name]


@pytest.mark.parametrize("name,k", CASES)
def test_solve_again_matches_the_refined_solution(name, k):
    c, lam, eta, dv = _open(name)
    assert c.info("FACTOR_KEPT") == 0
    e_base = _baseline_err(name, c, dv)[:k]
    B, Xref = sar.rhs_columns(name)[:, :k], sar.rhs_reference(name)[:, :k]
    st, x_eta = _factor(c, dv, eta)
    assert st == 0 and c.info("FACTOR_KEPT") == 1
    X = _solve(c, dv, B)
    assert c.info("FACTOR_KEPT") == 1, "a solve on the kept factor must keep it"
    res = np.array([np.linalg.norm(lam.matvec(X[:, j]) - B[:, j]) / np.linalg.norm(B[:, j]) for j in range(k)])
    print("%s k %d: largest residual %.3e (bound %.0e)" % (name, k, res.max(), RES_TOL))
    assert np.all(res < RES_TOL), res
    sar.check_criterion(sar.col_err(X, Xref), e_base, "%s k %d" % (name, k))
    dv.free()
    c.close()


@pytest.mark.parametrize("name,cols", [("edges32", (0, 15, 16, 127, 128)), ("loop73", (0, 2, 3, 16)), ("edges63_long", (1, 3, 16))])
def test_a_column_has_the_bits_of_that_column_solved_alone(name, cols):
    c, lam, eta, dv = _open(name)
    B = sar.rhs_columns(name)
    assert _factor(c, dv, eta)[0] == 0
    X = _solve(c, dv, B)
    assert np.array_equal(X, _solve(c, dv, B, ldb=lam.n)), "two runs differ"
    for j in cols:
        assert np.array_equal(_solve(c, dv, B[:, j:j + 1])[:, 0], X[:, j]), "column %d depends on its neighbours or its position" % j
    dv.free()
    c.close()


def _own_S(c):
    n = c.schur_buffer_size()
    out = np.empty(n)
    c._check(c.lib.spp_memcpy_d2h(c.h, out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(c.info("S_DEVICE_PTR")), out.nbytes))
    return out


@pytest.mark.parametrize("name", ["edges63", "loop73"])
def test_the_kept_state_is_not_disturbed(name):
    """factor(eta), solve_device, factor(eta): the second factor_solve gives the first one's bits, and the own S buffer ends
    as after two plain solves"""
    c, lam, eta, dv = _open(name)
    st, x1 = _factor(c, dv, eta)
    _solve(c, dv, sar.rhs_columns(name)[:, :6])
    st2, x2 = _factor(c, dv, eta)
    assert st == 0 and st2 == 0 and np.array_equal(x1, x2)
    S_with = _own_S(c)
    dv.free()
    c.close()
    c, lam, eta, dv = _open(name)
    _factor(c, dv, eta)
    st, x3 = _factor(c, dv, eta)
    assert np.array_equal(x3, x1)
    assert np.array_equal(S_with, _own_S(c), equal_nan=True), "the solve on the kept factor left a trace in the S buffer"
    dv.free()
    c.close()


def _refused(c, dv, n, code):
    """spp_solve_device and spp_marginals_device both answer `code`, and FACTOR_KEPT reads 0"""
    dB = api.DeviceArray.from_host(c, np.ones(n))
    dC = api.DeviceArray(c, 64)
    v = np.zeros(1, dtype=np.int64)
    assert c.lib.spp_solve_device(c.h, dv.ptr, dB.ptr, n, 1) == code
    assert c.lib.spp_marginals_device(c.h, dv.ptr, 1, v.ctypes.data_as(ctypes.c_void_p), dC.ptr) == code
    assert np.array_equal(dB.download(), np.ones(n)), "a refused call wrote to B"
    out = ctypes.c_int64(-1)
    assert c.lib.spp_get_info(c.h, api.INFO["FACTOR_KEPT"], ctypes.byref(out)) == 0 and out.value == 0
    dB.free(); dC.free()


def _usable(c, lam, eta, dv):
    """the ctx (analyzed in the dense Schur mode) still factors and solves again"""
    st, x = _factor(c, dv, eta)
    assert st == 0 and c.info("FACTOR_KEPT") == 1
    X = _solve(c, dv, eta[:, None])
    assert np.linalg.norm(lam.matvec(X[:, 0]) - eta) / np.linalg.norm(eta) < RES_TOL


def test_refused_without_a_kept_factor_and_the_ctx_stays_usable():
    name = "edges73_aligned"
    lam, eta = sar.problem(name)
    c = api.Context(0)
    dv = api.DeviceArray.from_host(c, lam.vals)
    _refused(c, dv, lam.n, E_STATE)                      # before any analysis
    c.analyze(lam, api.MODE_SCHUR)
    _refused(c, dv, lam.n, E_STATE)                      # before any factor
    _usable(c, lam, eta, dv)
    # after a factor that is not positive definite (the construction of test_indefinite_landmark_returns_false_and_keeps_eta)
    vals = lam.vals.copy()
    lm = int(np.flatnonzero(lam.dim == 3)[17])
    p = lam.col_ptr[lm + 1] - 1
    C = vals[lam.blk_off[p]:lam.blk_off[p] + 9].reshape(3, 3)
    ev = np.linalg.eigvalsh(C)
    C -= 0.5 * (ev[0] + ev[1]) * np.eye(3)
    dbad = api.DeviceArray.from_host(c, vals)
    assert _factor(c, dbad, eta)[0] == api.SPP_NOT_POSDEF
    _refused(c, dv, lam.n, E_STATE)
    dbad.free()
    _usable(c, lam, eta, dv)
    c.analyze(lam, api.MODE_SCHUR)                       # after analyze
    _refused(c, dv, lam.n, E_STATE)
    _usable(c, lam, eta, dv)
    A = np.eye(5) * 3.0                                  # after spp_dense_posv
    dA, db = api.DeviceArray.from_host(c, A.ravel()), api.DeviceArray.from_host(c, np.ones(5))
    assert c._check(c.lib.spp_dense_posv(c.h, dA.ptr, 5, 5, db.ptr)) == 0
    dA.free(); db.free()
    _refused(c, dv, lam.n, E_STATE)
    _usable(c, lam, eta, dv)
    dS = api.DeviceArray(c, c.schur_buffer_size())       # after the split form, on a caller's buffer too
    dr = api.DeviceArray.from_host(c, eta)
    c.schur_form(dv.ptr, dr.ptr, dS.ptr)
    _refused(c, dv, lam.n, E_STATE)
    assert c.schur_finish(dv.ptr, dS.ptr, dr.ptr) == 0
    _refused(c, dv, lam.n, E_STATE)
    dS.free(); dr.free()
    _usable(c, lam, eta, dv)
    dv.free()
    c.close()


@pytest.mark.parametrize("name,mode", [("edges73_aligned", api.MODE_SPARSE), ("edges73_aligned", api.MODE_SCHUR_SPARSE),
                                       ("mis33", api.MODE_SCHUR_MIS)])
def test_unsupported_modes_are_refused(name, mode):
    c, lam, eta, dv = _open(name, mode)
    assert _factor(c, dv, eta)[0] == 0
    _refused(c, dv, lam.n, E_UNSUPPORTED)
    st, x = _factor(c, dv, eta)                          # the ctx goes on solving in its own mode
    assert st == 0 and np.linalg.norm(lam.matvec(x) - eta) / np.linalg.norm(eta) < 1e-10
    dv.free()
    c.close()


def test_a_sharded_ctx_is_refused():
    lam, eta = sar.problem("tiny_shards")
    c = api.Context(0)
    c.set_shard(0, 2)
    c.analyze(lam, api.MODE_SCHUR)
    dv = api.DeviceArray.from_host(c, lam.vals)
    _refused(c, dv, lam.n, E_UNSUPPORTED)
    dv.free()
    c.set_shard(0, 1)                                    # back to one shard: set_shard drops nothing it should keep
    c.analyze(lam, api.MODE_SCHUR)
    dv = api.DeviceArray.from_host(c, lam.vals)
    _usable(c, lam, eta, dv)
    c.set_shard(0, 1)
    assert c.info("FACTOR_KEPT") == 0, "spp_set_shard must drop the kept factor"
    dv.free()
    c.close()


def test_bad_arguments_leave_the_factor_kept():
    c, lam, eta, dv = _open("tiny_shards")
    assert _factor(c, dv, eta)[0] == 0
    n = lam.n
    dB = api.DeviceArray.from_host(c, np.ones(2 * n))
    dC = api.DeviceArray(c, 64 * 64)
    lib, h = c.lib, c.h
    assert lib.spp_solve_device(h, dv.ptr, dB.ptr, n, 0) == E_BADARG          # nrhs < 1
    assert lib.spp_solve_device(h, dv.ptr, dB.ptr, n - 1, 1) == E_BADARG      # ldb < n
    assert lib.spp_solve_device(h, None, dB.ptr, n, 1) == E_BADARG
    assert lib.spp_solve_device(h, dv.ptr, None, n, 1) == E_BADARG

    def marg(vs):
        v = np.asarray(vs, dtype=np.int64)
        return lib.spp_marginals_device(h, dv.ptr, v.size, v.ctypes.data_as(ctypes.c_void_p), dC.ptr)
    assert marg([0, 1, 0]) == E_BADARG                                         # a repeated vertex
    assert marg([lam.nb]) == E_BADARG and marg([-1]) == E_BADARG               # out of range
    assert lib.spp_marginals_device(h, dv.ptr, 0, np.zeros(1, np.int64).ctypes.data_as(ctypes.c_void_p), dC.ptr) == E_BADARG
    assert lib.spp_marginals_device(h, dv.ptr, 1, None, dC.ptr) == E_BADARG
    assert np.array_equal(dB.download(), np.ones(2 * n))
    assert c.info("FACTOR_KEPT") == 1
    X = _solve(c, dv, eta[:, None])
    assert np.linalg.norm(lam.matvec(X[:, 0]) - eta) / np.linalg.norm(eta) < RES_TOL
    dB.free(); dC.free(); dv.free()
    c.close()
