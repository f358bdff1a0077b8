"""Self-calibrating bundle adjustment resident on the device (nonlinear._ResidentBAIPath): one damped iteration through
spp_ba_intrinsics_linearize_device, spp_assemble_ternary_device and spp_factor_solve_device (AUTO: the dense Schur mode, poses
= cameras + intrinsics) against a float64 solve of the mirror's padded Lambda; the Levenberg-Marquardt loop against the same
loop on the host; a rejected step."""
import numpy as np
import pytest

from slam_plus_plus_amd import api, nonlinear
import bai_cases as bc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", bc.FIXTURES)
def test_one_resident_iteration(name):
    """dx within 1e-10 relative of a float64 direct solve of the mirror's padded Lambda with the same damping; the inert
    entries of dx exactly 0. bai_tiny and bai_small: dense LAPACK. bai_hub (9246 unknowns) deviates from the dense solve
    the feature's specification names: a dense factorization of 0.7 GB takes tens of seconds on the host, so there the
    reference is SuperLU on the same float64 matrix, points eliminated first, no pivoting off the diagonal
    (bai_cases.solve_padded) -- still a direct float64 solve that shares nothing with the device path; the bound is kept."""
    prob = bc.fixture(name)
    s = nonlinear.CBundleAdjustmentIntrinsics.from_problem(prob)
    p = nonlinear._ResidentBAIPath(0)
    p.begin(s)
    p.linearize()
    alpha = 1e-3 * p.max_hessian_diag()
    host = bc.HostBAIPath()
    host.begin(s)
    host.linearize()
    alpha_h = 1e-3 * host.max_hessian_diag()
    assert abs(alpha - alpha_h) <= 1e-12 * alpha_h
    ok, norm = p.solve(alpha)
    assert ok and p.ctx.info("MODE") == api.MODE_SCHUR and p.ctx.info("N_POSES") == prob.nc + prob.ni
    dx, eta = p.d_dx.download(), p.d_eta.download()
    denom = p.gain_denominator(alpha)
    p.close()
    lam, eta_h = bc.padded_lambda(prob, alpha)
    want = bc.solve_padded(lam, eta_h, prob.dim)
    rel = np.linalg.norm(dx - want) / np.linalg.norm(want)
    print(name, "alpha %.6g, dx relative difference to the float64 solve: %.3e" % (alpha, rel))
    assert np.abs(eta - eta_h).max() <= 1e-11 * np.abs(eta_h).max()
    assert rel <= 1e-10
    inert = s.intr_off + 5
    assert not dx[inert].any() and not eta[inert].any()
    assert abs(norm - np.linalg.norm(dx)) <= 1e-12 * np.linalg.norm(dx)
    assert abs(denom - dx @ (alpha * dx + eta)) <= 1e-10 * abs(denom)


class _Traced(nonlinear._ResidentBAIPath):
    """the resident path, recording which steps the loop kept (save) and which it rolled back (restore)"""

    def begin(self, system):
        super().begin(system)
        self.trace = []

    def save(self):
        super().save()
        self.trace.append(True)

    def restore(self):
        super().restore()
        self.trace[-1] = False


@pytest.mark.parametrize("name", bc.FIXTURES)
def test_resident_lm_matches_the_host_loop(name):
    """CNonlinearSolver_Lambda_LM (unchanged) with _ResidentBAIPath against the same loop on the host path, 5 iterations:
    the same accepted steps, the final states within 1e-6 max(1, |x|), the final chi2 to 1e-9 relative"""
    host, hs = bc.host_lm(name, 5, 1e-4)
    dev = nonlinear.CBundleAdjustmentIntrinsics.from_problem(bc.fixture(name))
    ds = nonlinear.CNonlinearSolver_Lambda_LM(dev, path=_Traced())
    ds.Optimize(5, 1e-4)
    assert ds.path.ctx.info("MODE") == api.MODE_SCHUR
    ds.path.close()
    print(name, "steps kept:", ds.path.trace, "chi2:", ["%.9g" % c for c in ds.chi2_history])
    assert ds.path.trace == hs.path.trace and ds.n_iterations == hs.n_iterations == 5
    assert hs.chi2_history[-1] < 0.05 * hs.chi2_history[0]
    for a, b in zip(dev.state(), host.state()):
        d = np.abs(a - b) / np.maximum(1.0, np.abs(b))
        print(name, "max state difference to the host loop: %.3e max(1, |x|)" % d.max())
        assert d.max() <= 1e-6
    assert abs(dev.chi2() - host.chi2()) <= 1e-9 * host.chi2()
    assert abs(ds.chi2_history[-1] - hs.chi2_history[-1]) <= 1e-9 * hs.chi2_history[-1]


class _HugeFirstStep(_Traced):
    """multiplies the first increment by 200: the step is rejected; snapshots the states after the roll-back"""

    def apply(self):
        if not self.trace[:-1]:
            self.d_dx.upload(200.0 * self.d_dx.download())
        super().apply()

    def restore(self):
        super().restore()
        self.ctx.synchronize()
        self.after = [a.download() for a in (self.d_cams, self.d_pts, self.d_intr)]


def test_a_rejected_step_restores_every_state_bit_for_bit():
    s = nonlinear.CBundleAdjustmentIntrinsics.from_problem(bc.fixture("bai_small"))
    x0 = s.state()
    path = _HugeFirstStep()
    solver = nonlinear.CNonlinearSolver_Lambda_LM(s, path=path)
    solver.Optimize(3, 1e-4)
    path.close()
    print("steps kept:", path.trace, "chi2:", solver.chi2_history)
    assert path.trace[0] is False and any(path.trace[1:])
    for got, want in zip(path.after, (x0[0], x0[1], x0[2])):
        assert np.array_equal(got, want.ravel())
    assert solver.chi2_history[-1] < solver.chi2_history[0]
