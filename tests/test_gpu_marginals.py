"""GPU: spp_marginals_device -- the joint covariance E^T Lambda^-1 E of chosen vertices as one solve with unit block
columns on the kept factor. Checked against refined unit-column solves (tests/solve_again_ref.py) with the criterion of
tests/test_gpu_solve_again.py: per column, error <= max(1e-10, 4 x the error of spp_factor_solve_device on the same unit
column), both measured on the selected rows."""
import numpy as np
import pytest

import schur_fixtures as fx
import solve_again_ref as sar
from slam_plus_plus_amd import api

pytestmark = pytest.mark.gpu

N_TWO = sum(k for _, _, k in fx.PAIR_SPREAD)   # the two-observer landmarks come first


def _selection(name):
    """vertices (block columns) of the fixture, shuffled: first and last camera (the last one observes nothing), a camera
    straddling the first 128-row boundary, a degree-1 landmark, the 256-track's landmark where there is one, an unobserved
    landmark"""
    lam = sar.problem(name)[0]
    dp = int(lam.dim.max())
    nc = int(np.count_nonzero(lam.dim == dp))
    straddle = 128 // dp
    assert lam.base[straddle] < 128 < lam.base[straddle + 1]
    sel = [0, nc - 1, nc - 2, straddle, nc + N_TWO, nc + N_TWO + fx.N_SINGLE + 7]
    if name == "edges63":
        sel.append(nc + N_TWO + fx.N_SINGLE + fx.N_SPARSE)
    return [sel[i] for i in np.random.default_rng(5).permutation(len(sel))], nc - 1


@pytest.mark.parametrize("name", ["edges63", "edges73_aligned"])
def test_joint_covariance_matches_the_refined_unit_columns(name):
    lam, eta = sar.problem(name)
    sel, cam_blind = _selection(name)
    cov_ref, Xref, rows = sar.covariance_ref(name, sel)
    c = api.Context(0)
    c.analyze(lam, api.MODE_SCHUR)
    dv = api.DeviceArray.from_host(c, lam.vals)
    E, _ = sar.unit_columns(lam, sel)
    base = sar.baseline_columns(c, dv.ptr, E)[rows]      # the existing path on the same unit columns
    dr = api.DeviceArray.from_host(c, eta)
    assert c.factor_solve_device(dv.ptr, dr.ptr) == 0
    cov = c.marginals(dv.ptr, sel)
    assert c.info("FACTOR_KEPT") == 1
    m = rows.size
    assert cov.shape == (m, m)
    assert np.array_equal(cov, cov.T), "not exactly symmetric"
    sar.check_criterion(sar.col_err(cov, cov_ref), sar.col_err(base, cov_ref), "%s covariance of %d vertices" % (name, len(sel)))
    at = 0
    for v in sel:
        d = int(lam.dim[v])
        np.linalg.cholesky(cov[at:at + d, at:at + d])   # (raises unless positive definite)
        at += d
    # a single vertex's marginal is the corresponding block of the joint one, bit for bit (a camera, the blind camera, a landmark)
    at = 0
    for v in sel:
        d = int(lam.dim[v])
        if v in (sel[0], cam_blind, sel[-1], 0):
            assert np.array_equal(c.marginals(dv.ptr, [v]), cov[at:at + d, at:at + d]), "vertex %d" % v
        at += d
    # and twice the same
    assert np.array_equal(c.marginals(dv.ptr, sel), cov)
    dv.free(); dr.free()
    c.close()
