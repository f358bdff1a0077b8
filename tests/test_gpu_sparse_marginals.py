"""GPU: spp_sparse_marginals_device -- the joint covariance E^T Lambda^-1 E of chosen vertices of a pose graph as one solve
with unit block columns on the kept sparse factor. Checked against refined unit-column solves (tests/sparse_solve_ref.py)
with the criterion of tests/test_gpu_sparse_solve_again.py: per column, error <= max(1e-10, 4 x the error of
spp_factor_solve_device on the same unit column), both measured on the selected rows.

Designed systems (small_trees, tree_hi, chain): one block of the first leaf, of the widest leaf and of the separator, plus a
width-1 and a width-8 block, shuffled. The damped pose graphs (se2_small, se3_small): the first, middle and last pose and
two adjacent ones."""
import numpy as np
import pytest

import solve_again_ref as sar
import sparse_solve_ref as ssr
from slam_plus_plus_amd import api

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["small_trees", "tree_hi", "chain", "se2_small", "se3_small"])
def test_joint_covariance_matches_the_refined_unit_columns(name):
    lam, eta = ssr.problem(name)
    sel = ssr.marginal_selection(name)
    cov_ref, Xref, rows = ssr.covariance_ref(name, sel)
    c = api.Context(0)
    c.analyze(lam, api.MODE_SPARSE)
    dv = api.DeviceArray.from_host(c, lam.vals)
    E, _ = sar.unit_columns(lam, sel)
    base = sar.baseline_columns(c, dv.ptr, E)[rows]      # the existing path on the same unit columns
    dr = api.DeviceArray.from_host(c, eta)
    assert c.factor_solve_device(dv.ptr, dr.ptr) == 0
    x_eta = dr.download()
    cov = c.sparse_marginals(sel)
    assert c.info("SPARSE_FACTOR_KEPT") == 1 and c.info("FACTOR_KEPT") == 0
    m = rows.size
    assert cov.shape == (m, m)
    assert np.array_equal(cov, cov.T), "not exactly symmetric"
    sar.check_criterion(sar.col_err(cov, cov_ref), sar.col_err(base, cov_ref), "%s covariance of %d vertices" % (name, len(sel)))
    at = 0
    for v in sel:
        d = int(lam.dim[v])
        np.linalg.cholesky(cov[at:at + d, at:at + d])   # (raises unless positive definite)
        assert np.array_equal(c.sparse_marginals([v]), cov[at:at + d, at:at + d]), "vertex %d alone" % v
        at += d
    # twice the same, and the factorization that follows is not disturbed
    assert np.array_equal(c.sparse_marginals(sel), cov)
    dr.upload(eta)
    assert c.factor_solve_device(dv.ptr, dr.ptr) == 0
    assert np.array_equal(dr.download(), x_eta)
    dv.free(); dr.free()
    c.close()
