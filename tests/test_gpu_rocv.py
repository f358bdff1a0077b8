"""Resident Gauss-Newton on range-only constant-velocity graphs (nonlinear.CRocv, _ResidentROCVPath): the whole iteration in
HBM -- spp_rocv_cv_linearize_device, spp_rocv_range_linearize_device, the priors as a unary group, spp_assemble_groups_device,
spp_factor_solve_device in the sparse and in the Schur mode, the plain update -- against the numpy loop with a dense float64
solve (tests/rocv_ref.py). rocv_small: 40 receivers, 5 transmitters; rocv_interleaved: 150 + 8 with the transmitters' ids
among the receivers', every transmitter and one receiver beyond 24 sources (both wave kernels run)."""
import numpy as np
import pytest

import rocv_ref
from slam_plus_plus_amd import api, nonlinear, synth

pytestmark = pytest.mark.gpu
FIXTURES = ["rocv_small", "rocv_interleaved"]
MODES = [api.MODE_SPARSE, api.MODE_SCHUR]


def _system(name):
    return nonlinear.CRocv.from_problem(synth.make(name))


def _close(state, ref):
    return np.abs(state - ref).max() <= 1e-6 * max(1.0, np.abs(ref).max())   # the bound of DESIGN section 15


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", FIXTURES)
def test_resident_gauss_newton_matches_the_numpy_loop(name, mode):
    ref_state, ref_it, ref_norms = rocv_ref.host_result(name)
    s = _system(name)
    path = nonlinear._ResidentROCVPath(0, mode=mode)
    solver = nonlinear.CNonlinearSolver_Lambda(s, path=path)
    n_it = solver.Optimize(5, 0.01)
    info_mode = path.ctx.info("MODE")
    path.close()
    print(name, "mode", info_mode, "iterations", n_it, "last norm %.3e (numpy %.3e)" % (solver.last_dx_norm, ref_norms[-1]),
          "max state difference %.3e" % np.abs(s.state - ref_state).max())
    assert info_mode == mode
    assert n_it == ref_it and solver.last_dx_norm <= 0.01
    assert _close(s.state, ref_state)


def test_default_path_and_host_jacobians_agree(hip_ctx):
    """CNonlinearSolver_Lambda picks the resident path for a CRocv; host_jacobians=True sends the numpy mirror's three
    groups (the unary one with an empty J1) through _DeviceGroupsPath unchanged"""
    for name in FIXTURES:
        ref_state, ref_it, _ = rocv_ref.host_result(name)
        a, b = _system(name), _system(name)
        sa = nonlinear.CNonlinearSolver_Lambda(a)
        assert isinstance(sa.path, nonlinear._ResidentROCVPath) and sa.path.mode == api.MODE_SPARSE
        sb = nonlinear.CNonlinearSolver_Lambda(b, host_jacobians=True)
        assert type(sb.path) is nonlinear._DeviceGroupsPath
        na, nb = sa.Optimize(5, 0.01), sb.Optimize(5, 0.01)
        sa.path.close(), sb.path.close()
        assert na == nb == ref_it
        assert _close(a.state, b.state) and _close(a.state, ref_state)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", FIXTURES)
def test_first_increment_against_a_dense_solve(name, mode):
    """dx of the first iteration in both solver modes within 1e-10 relative of numpy's solve of the mirror's dense Lambda;
    the device's chi2 (rd 6 + rd 1; the priors' is 0) against the mirror's"""
    s = _system(name)
    L, eta = rocv_ref.dense_lambda(s.linearize())
    dx_ref = np.linalg.solve(L, eta)
    path = nonlinear._ResidentROCVPath(0, mode=mode)
    path.begin(s)
    chi2 = path.chi2()
    ok, norm = path.step()
    dx = path.d_eta.download()
    path.close()
    rel = np.linalg.norm(dx - dx_ref) / np.linalg.norm(dx_ref)
    print(name, "mode", mode, "relative dx difference %.3e, chi2 %.6f / %.6f" % (rel, chi2, s.chi2()))
    assert ok and rel <= 1e-10
    assert abs(norm - np.linalg.norm(dx_ref)) <= 1e-10 * np.linalg.norm(dx_ref)
    assert abs(chi2 - s.chi2()) <= 1e-12 * s.chi2()
