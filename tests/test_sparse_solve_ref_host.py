"""CPU: the reference machinery of tests/test_gpu_sparse_solve_again.py and tests/test_gpu_sparse_marginals.py, checked
without a GPU.

  - sparse_solve_ref.refined_columns on eta is sparse_fixtures.reference (designed fixtures) / parity.refined_solution (pose
    graphs) bit for bit: the same operations in the same order, the factor computed once.
  - E^T Lambda^-1 E assembled from refined unit columns agrees with the longdouble Gauss-Jordan inverse of Lambda to
    64 cond eps, cond measured (small_trees, chain: per connected component; se3_small: the dense Lambda, 576 x 576).
  - cond_2 <= 100 on every designed fixture (80 by construction), and cond(Lambda) of the two pose graphs at damping 50
    below solve_again_ref.COND_MAX: the refined columns are then exact to ~cond eps^2, far below the 1e-10 floor of the
    criterion."""
import numpy as np
import pytest

import parity
import solve_again_ref as sar
import sparse_fixtures as sf
import sparse_solve_ref as ssr
from test_solve_again_ref_host import _ld_solve

EPS = float(np.finfo(np.float64).eps)


@pytest.mark.parametrize("name", ["small_trees", "forest_a", "se2_small"])
def test_refined_columns_are_the_existing_references_bit_for_bit(name):
    lam, eta = ssr.problem(name)
    B = ssr.rhs_columns(name)
    assert np.array_equal(B[:, 0], eta)
    assert np.count_nonzero(B[:, 2]) == 1 and np.count_nonzero(B[:, 3]) == 1
    x = ssr.refined_columns(name, B[:, :1])[:, 0]
    if name in ssr.POSE:
        assert np.array_equal(x, parity.refined_solution(lam, eta))
    else:
        assert np.array_equal(x, sf.reference(ssr.fixture(name))[0])


def test_unit_rows_stand_in_a_leaf_and_in_a_separator():
    for name in sf.NAMES:
        fx = ssr.fixture(name)
        lam = fx.lam
        r_leaf, r_sep = ssr.leaf_and_separator_rows(name)
        role = {}
        for g in fx.cliques:
            for v in g["blocks"]:
                role[int(v)] = g["role"]
        block_of = np.searchsorted(lam.base, [r_leaf, r_sep], side="right") - 1
        assert role[int(block_of[0])] == "leaf" and role[int(block_of[1])] == "separator", name


def _exact_inverse_columns(name, E):
    lam = ssr.problem(name)[0]
    if name in ssr.POSE:
        return _ld_solve(lam.to_scipy().toarray(), E)
    fx = ssr.fixture(name)
    X = np.zeros(E.shape, dtype=np.longdouble)
    for s, L in zip(fx.comp_scalars, fx.dense):
        X[s] = _ld_solve(L, E[s])
    return X


@pytest.mark.parametrize("name", ["small_trees", "chain", "se3_small"])
def test_covariance_from_refined_unit_columns_matches_the_longdouble_inverse(name):
    lam = ssr.problem(name)[0]
    sel = ssr.marginal_selection(name)
    assert len(set(sel)) == len(sel) == 5
    if name not in ssr.POSE:
        assert {1, 8} <= set(int(d) for d in lam.dim[sel])
    cov, X, rows = ssr.covariance_ref(name, sel)
    E, _ = sar.unit_columns(lam, sel)
    exact = _exact_inverse_columns(name, E)
    cond = ssr.condition(name)
    bound = 64 * cond * EPS
    err = np.linalg.norm((X - exact).astype(np.float64), axis=0) / np.linalg.norm(exact.astype(np.float64), axis=0)
    err_cov = float(np.abs(cov - exact[rows].astype(np.float64)).max() / np.abs(exact[rows]).max())
    print("%s: cond %.3e, largest column error %.3e, covariance block error %.3e, bound %.3e" % (name, cond, err.max(), err_cov, bound))
    assert np.all(err <= bound) and err_cov <= bound
    assert float(np.abs(cov - cov.T).max()) <= bound * float(np.abs(cov).max())


@pytest.mark.parametrize("name", sf.NAMES)
def test_every_designed_fixture_is_well_conditioned(name):
    cond = ssr.condition(name)
    print("%s: cond_2 = %.3e" % (name, cond))
    assert cond <= 100.0


@pytest.mark.parametrize("name", ssr.POSE)
def test_the_damped_pose_graphs_are_well_conditioned(name):
    cond = ssr.condition(name)
    print("%s at damping %g: cond(Lambda) = %.3e" % (name, ssr.POSE_DAMPING, cond))
    assert cond < sar.COND_MAX
