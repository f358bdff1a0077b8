"""Sim(3) bundle adjustment on the device: the resident Levenberg-Marquardt loop (nonlinear._ResidentSim3BAPath:
spp_sim3_ba_linearize_device, assembly (7, 3, 2), the Schur solve with 7-wide cameras, spp_sim3_update_device) against the
same loop on the host (the float64 mirror's Jacobians, a numpy dense solve), with the device's and with the mirror's
Jacobians; the first step against numpy's dense solve."""
import functools

import numpy as np
import pytest

from slam_plus_plus_amd import api, nonlinear, synth
import sim3_cases as sc

pytestmark = pytest.mark.gpu
FIXTURES = ["sim3_small", "sim3_interleaved"]


class _Traced(nonlinear._ResidentSim3BAPath):
    """the resident path, recording which steps the loop kept (save) and which it rolled back (restore), and the first dx"""

    def begin(self, system):
        super().begin(system)
        self.trace = []
        self.first_dx = None

    def solve(self, alpha):
        out = super().solve(alpha)
        if self.first_dx is None:
            self.first_dx = self.d_dx.download()
        return out

    def save(self):
        super().save()
        self.trace.append(True)

    def restore(self):
        super().restore()
        self.trace[-1] = False


@functools.lru_cache(maxsize=None)
def host_loop(name):
    """the host loop of a fixture, run once and shared: (system, solver)"""
    host = nonlinear.CBundleAdjustmentSim3.from_problem(synth.make(name))
    hs = nonlinear.CNonlinearSolver_Lambda_LM(host, path=sc.HostSim3Path())
    hs.Optimize(8, 1e-4)
    return host, hs


@pytest.mark.parametrize("host_jacobians", [False, True])
@pytest.mark.parametrize("name", FIXTURES)
def test_resident_lm_matches_the_host_loop(name, host_jacobians):
    host, hs = host_loop(name)
    dev = nonlinear.CBundleAdjustmentSim3.from_problem(synth.make(name))
    ds = nonlinear.CNonlinearSolver_Lambda_LM(dev, path=_Traced(host_jacobians=host_jacobians))
    ds.Optimize(8, 1e-4)
    assert ds.path.ctx.info("MODE") == api.MODE_SCHUR
    assert ds.path.ctx.info("N_REDUCED") == 7 * dev.cams.shape[0]
    ds.path.close()
    print(name, "steps kept:", ds.path.trace, "chi2:", ["%.9g" % c for c in ds.chi2_history])
    assert ds.path.trace == hs.path.trace and ds.n_iterations == hs.n_iterations and len(ds.path.trace) >= 2
    assert hs.chi2_history[-1] < 0.05 * hs.chi2_history[0]
    d1 = np.abs(ds.path.first_dx - hs.path.first_dx).max() / np.abs(hs.path.first_dx).max()
    print(name, "first dx against numpy's dense solve: %.3e" % d1)
    assert d1 <= 1e-10
    for a, b in zip(dev.state(), host.state()):
        d = np.abs(a - b).max()
        print(name, "max state difference to the host loop: %.3e" % d)
        assert d <= 1e-6 * max(1.0, np.abs(b).max())
    assert abs(dev.chi2() - host.chi2()) <= 1e-9 * host.chi2()
    assert abs(ds.chi2_history[-1] - hs.chi2_history[-1]) <= 1e-9 * hs.chi2_history[-1]
