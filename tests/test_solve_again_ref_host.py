"""CPU: the reference machinery of tests/test_gpu_solve_again.py and tests/test_gpu_marginals.py, checked without a GPU.

  - solve_again_ref.refined_columns is tests/parity.py's refined_solution with the LU shared: the same bits, column by column.
  - E^T Lambda^-1 E assembled from refined unit columns agrees with the longdouble inverse of Lambda to 64 cond eps, with
    cond computed: on tiny_shards against the Gauss-Jordan inverse of the dense Lambda (30 x 30) in longdouble; on edges32
    (n = 23 314: a dense longdouble Lambda would be 8.7 GB) against the same inverse evaluated by blocks -- with
    Lambda = [A U; U^T C], Lambda^-1 e = [x_c; C^-1 (e_l - U^T x_c)], x_c = S^-1 (e_c - U C^-1 e_l) -- from the longdouble
    S, C^-1 and U of tests/schur_ref.py and a longdouble Gauss-Jordan solve with S; tiny_shards checks that route against
    the dense one.
  - every fixture of the GPU tests (sar.FIXTURES and sar.SCHEDULE_FIXTURES) has cond(Lambda) < 1e6: the refined solutions are then exact to ~cond eps^2 < 1e-25
    relative, far below the 1e-10 floor of the criterion."""
import numpy as np
import pytest

import parity
import schur_ref
import solve_again_ref as sar

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)


def _ld_solve(A, B):
    """A^-1 B in longdouble: Gauss-Jordan with partial pivoting"""
    a = np.concatenate([A.astype(LD), B.astype(LD)], axis=1)
    n = A.shape[0]
    for k in range(n):
        p = k + int(np.argmax(np.abs(a[k:, k])))
        if p != k:
            a[[k, p]] = a[[p, k]]
        a[k] /= a[k, k]
        f = a[:, k].copy()
        f[k] = 0
        a -= f[:, None] * a[k][None, :]
    return a[:, n:]


def _inverse_columns_by_blocks(lam, E):
    """Lambda^-1 E in longdouble through the landmark elimination (never a dense Lambda)"""
    elim = schur_ref.guided_elim(lam)
    R = schur_ref.schur_ref(lam, np.zeros(lam.n), elim)
    dp, dl = R.dp, R.dl
    pidx = schur_ref.pose_index(lam, R.poses)
    lidx = lam.base[R.lms][:, None] + np.arange(dl)[None, :]
    U = R.obs_B.astype(LD)                                   # (observations, dp, dl)
    m = E.shape[1]
    El = E[lidx].astype(LD)                                  # (nl, dl, m)
    CiEl = np.einsum("lde,lem->ldm", R.Cinv, El)
    P = E[pidx].astype(LD).reshape(R.poses.size, dp, m)
    np.subtract.at(P, R.obs_pose, np.einsum("ord,odm->orm", U, CiEl[R.obs_lm]))
    Xc = _ld_solve(R.S, P.reshape(R.n_red, m))
    T = El.copy()
    np.subtract.at(T, R.obs_lm, np.einsum("ord,orm->odm", U, Xc.reshape(R.poses.size, dp, m)[R.obs_pose]))
    Xl = np.einsum("lde,lem->ldm", R.Cinv, T)
    X = np.zeros((lam.n, m), dtype=LD)
    X[pidx] = Xc
    X[lidx.ravel()] = Xl.reshape(-1, m)
    return X


def _selection(lam):
    cams = np.flatnonzero(lam.dim == lam.dim.max())
    lms = np.flatnonzero(lam.dim == lam.dim.min())
    return [int(lms[-1]), int(cams[0]), int(lms[0]), int(cams[-1]), int(cams[cams.size // 2])]


def test_refined_columns_are_paritys_refined_solution_bit_for_bit():
    for name in ("tiny_shards", "edges32"):
        lam, eta = sar.problem(name)
        B = sar.rhs_columns(name)[:, :4]
        X = sar.refined_columns(name, B)
        for j in range(4):
            assert np.array_equal(X[:, j], parity.refined_solution(lam, np.ascontiguousarray(B[:, j]))), (name, j)
        assert np.array_equal(B[:, 0], eta)
        assert np.count_nonzero(B[:, 2]) == 1 and np.count_nonzero(B[:, 3]) == 1


def test_the_block_route_is_the_dense_longdouble_inverse_on_the_small_fixture():
    lam, _ = sar.problem("tiny_shards")
    E, rows = sar.unit_columns(lam, _selection(lam))
    dense = _ld_solve(lam.to_scipy().toarray(), E)
    blocks = _inverse_columns_by_blocks(lam, E)
    assert float(np.abs(dense - blocks).max() / np.abs(dense).max()) < 1e-17


@pytest.mark.parametrize("name", ["tiny_shards", "edges32"])
def test_covariance_from_refined_unit_columns_matches_the_longdouble_inverse(name):
    lam, _ = sar.problem(name)
    sel = _selection(lam)
    cov, X, rows = sar.covariance_ref(name, sel)
    E, _ = sar.unit_columns(lam, sel)
    if name == "tiny_shards":
        exact = _ld_solve(lam.to_scipy().toarray(), E)
    else:
        exact = _inverse_columns_by_blocks(lam, E)
    cond = sar.condition(name)
    bound = 64 * cond * EPS
    err = np.linalg.norm((X - exact).astype(np.float64), axis=0) / np.linalg.norm(exact.astype(np.float64), axis=0)
    err_cov = float(np.abs(cov - exact[rows].astype(np.float64)).max() / np.abs(exact[rows]).max())
    print("%s: cond %.3e, largest column error %.3e, covariance block error %.3e, bound %.3e" % (name, cond, err.max(), err_cov, bound))
    assert np.all(err <= bound) and err_cov <= bound
    assert float(np.abs(cov - cov.T).max()) <= bound * float(np.abs(cov).max())


@pytest.mark.parametrize("name", sar.FIXTURES + [n for n in sar.SCHEDULE_FIXTURES if n not in sar.FIXTURES])
def test_every_fixture_of_the_gpu_tests_is_well_conditioned(name):
    cond = sar.condition(name)
    print("%s: cond(Lambda) = %.3e" % (name, cond))
    assert cond < sar.COND_MAX
