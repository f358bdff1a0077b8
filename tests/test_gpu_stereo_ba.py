"""Stereo bundle adjustment on the device: spp_ba_stereo_linearize_device (CBAJacobians::Project_P2SC as CEdgeP2SC3D calls
it) against the float64 mirror (formats.stereo_expectation / stereo_linearize), one damped iteration through assembly
(6, 3, 3), solve and spp_ba_update_device, the resident Levenberg-Marquardt loop (nonlinear._ResidentStereoBAPath) against
the same loop on the host, and the reference's application on the golden's file with the HIP solver behind it."""
import functools
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from slam_plus_plus_amd import api, formats, nonlinear, synth
from test_stereo_host import GOLD, HostStereoPath, edge_case_state

pytestmark = pytest.mark.gpu
FIXTURES = ["stereo_small", "stereo_interleaved"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _relmax(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@functools.lru_cache(maxsize=None)
def _edge_case_inputs():
    """64 observations of stereo_interleaved at the state of edge_case_state, the five cases in front; the mirror's
    linearization of exactly these, computed once"""
    p = synth.make("stereo_interleaved")
    cams, intr, pts, cases = edge_case_state(p)
    first = list(dict.fromkeys(cases.values()))
    sel = np.array(first + [k for k in range(p.v0.size) if k not in first][:64 - len(first)])
    obs = p.geometry["obs"][sel]
    g = formats.stereo_linearize(cams, intr, pts, obs)
    e = formats.stereo_expectation(cams[obs[:, 0].astype(int)], intr[obs[:, 0].astype(int)], pts[obs[:, 1].astype(int)])
    return cams, intr, pts, obs, g, e, {k: first.index(v) for k, v in cases.items()}


def _run_kernel(ctx, cams, intr, pts, cam_of, pt_of, meas):
    n = cam_of.size
    up = lambda a: api.DeviceArray.from_host(ctx, np.ascontiguousarray(a).ravel())
    out = [api.DeviceArray(ctx, w * n) for w in (18, 9, 3)]
    ctx.ba_stereo_linearize_device(n, up(cam_of.astype(np.int32)).ptr, up(pt_of.astype(np.int32)).ptr, up(cams).ptr,
                                   up(intr).ptr, up(pts).ptr, up(meas).ptr, *[o.ptr for o in out])
    ctx.synchronize()
    return [o.download().reshape(n, -1) for o in out]


def test_kernel_matches_the_numpy_mirror():
    """r within 1e-11 px of z - stereo_expectation (the mirror moves the point by -b (row 0 of R)^T as the reference does,
    the kernel evaluates x - b e0), J0 / J1 within 1e-12 relative of the mirror's analytic ones, the cases of
    edge_case_state each against their own block; a measurement offset comes back as r."""
    cams, intr, pts, obs, g, e, cases = _edge_case_inputs()
    n = obs.shape[0]
    ang = np.linalg.norm(cams[obs[:, 0].astype(int), 3:], axis=1)
    assert n == 64 and 0 < ang[cases["small"]] < 1e-10 and abs(ang[cases["pi"]] - np.pi) < 1e-3
    assert intr[int(obs[cases["d0"], 0]), 4] == 0 and intr[int(obs[cases["axis"], 0]), 4] != 0
    assert np.array_equal(e[cases["axis"], :2], intr[int(obs[cases["axis"], 0]), 2:4])       # rho = 0 exactly
    assert e[cases["axis_right"], 2] == intr[int(obs[cases["axis_right"], 0]), 2]            # rho_right = 0
    ctx = api.Context(0)
    J0, J1, r = _run_kernel(ctx, cams, intr, pts, obs[:, 0], obs[:, 1], obs[:, 2:5])
    assert np.isfinite(J0).all() and np.isfinite(J1).all() and np.isfinite(r).all()
    d_r = np.abs(r - (obs[:, 2:5] - e)).max()
    errs = [_relmax(J0, g.J0), _relmax(J1, g.J1)]
    print("r: %.3e px; J0, J1 relative max-abs: %.2e %.2e" % (d_r, errs[0], errs[1]))
    assert d_r <= 1e-11
    assert max(errs) <= 1e-12, errs
    for kc in cases.values():
        for o, w in ((J0, g.J0), (J1, g.J1)):
            assert np.abs(o[kc] - w[kc]).max() <= 1e-12 * max(1.0, np.abs(w[kc]).max()), kc
    off = np.array([0.25, -0.5, 0.125])
    _, _, r2 = _run_kernel(ctx, cams, intr, pts, obs[:, 0], obs[:, 1], e + off)
    assert np.abs(r2 - off).max() <= 1e-11
    ctx.close()


def test_gathered_indices_give_the_permuted_rows():
    cams, intr, pts, obs, _, _, _ = _edge_case_inputs()
    ctx = api.Context(0)
    a = _run_kernel(ctx, cams, intr, pts, obs[:, 0], obs[:, 1], obs[:, 2:5])
    perm = np.random.default_rng(0).permutation(obs.shape[0])
    b = _run_kernel(ctx, cams, intr, pts, obs[perm, 0], obs[perm, 1], obs[perm, 2:5])
    for x, y in zip(a, b):
        assert np.abs(x).max() > 0 and np.array_equal(y, x[perm])
    ctx.close()


@pytest.mark.parametrize("name", FIXTURES)
def test_resident_stereo_iteration_reduces_the_reprojection_error(name):
    """One damped Gauss-Newton (= LM with fixed damping) iteration entirely in HBM, the stereo twin of
    test_resident_ba_iteration_reduces_the_reprojection_error: device linearization -> device assembly (6, 3, 3) -> device
    solve -> device (+)."""
    from oracle import spp_oracle as orc
    prob = synth.make(name)
    s = synth.stereo_states(prob)
    no, nc, npts = prob.v0.size, s["cams"].shape[0], s["points"].shape[0]
    ctx = api.Context(0)
    st = ctx.assemble_analyze(prob.dim, prob.v0, prob.v1, 6, 3, 3, prob.unary_vertex)
    d = {k: api.DeviceArray.from_host(ctx, np.ascontiguousarray(v).ravel()) for k, v in s.items()}
    dOm = api.DeviceArray.from_host(ctx, prob.Om.ravel())
    J0, J1, r = api.DeviceArray(ctx, 18 * no), api.DeviceArray(ctx, 9 * no), api.DeviceArray(ctx, 3 * no)
    dv, de = api.DeviceArray(ctx, st.nvals), api.DeviceArray(ctx, st.n)

    def linearize():
        ctx.ba_stereo_linearize_device(no, d["cam_of"].ptr, d["pt_of"].ptr, d["cams"].ptr, d["intr"].ptr, d["points"].ptr,
                                       d["meas"].ptr, J0.ptr, J1.ptr, r.ptr)
        ctx.synchronize()
        return r.download().reshape(no, 3)

    r0 = linearize()
    assert np.abs(r0 - prob.r).max() < 1e-9
    damping = 1e-3 * ctx.edge_hessian_maxdiag_device(no, 3, 6, 3, J0.ptr, J1.ptr, dOm.ptr)
    assert abs(damping - prob.damping) <= 1e-12 * prob.damping
    ctx.assemble_device(J0.ptr, J1.ptr, dOm.ptr, r.ptr, damping, dv.ptr, de.ptr)
    lam, eta = st.with_vals(dv.download()), de.download()
    ctx.analyze(st, api.MODE_AUTO)
    assert ctx.factor_solve_device(dv.ptr, de.ptr) == 0
    dx = de.download()
    code, xo, _ = orc.schur_solve(lam, eta)
    assert code == 0 and np.linalg.norm(dx - xo) / np.linalg.norm(xo) < 1e-10
    nrm = ctx.ba_update_device(nc, d["cams"].ptr, d["cam_dxoff"].ptr, npts, d["points"].ptr, d["pt_dxoff"].ptr,
                               de.ptr, st.n, apply=True)
    assert abs(nrm - np.linalg.norm(dx)) <= 1e-12 * np.linalg.norm(dx)
    r1 = linearize()
    print(name, "sum r^2: %.6g -> %.6g" % ((r0 ** 2).sum(), (r1 ** 2).sum()))
    assert (r1 ** 2).sum() < 0.9 * (r0 ** 2).sum(), ((r0 ** 2).sum(), (r1 ** 2).sum())
    ctx.close()


class _Traced(nonlinear._ResidentStereoBAPath):
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


@pytest.mark.parametrize("name", FIXTURES)
def test_resident_lm_matches_the_host_loop(name):
    """CNonlinearSolver_Lambda_LM (unchanged) with _ResidentStereoBAPath against the same loop on the host path (numpy
    mirror, dense float64 solve): the same sequence of accepted and rejected steps, the final states within
    1e-6 max(1, |state|), the final chi2 to 1e-9 relative."""
    host = nonlinear.CStereoBundleAdjustment.from_problem(synth.make(name))
    hs = nonlinear.CNonlinearSolver_Lambda_LM(host, path=HostStereoPath())
    hs.Optimize(8, 1e-4)
    dev = nonlinear.CStereoBundleAdjustment.from_problem(synth.make(name))
    ds = nonlinear.CNonlinearSolver_Lambda_LM(dev, path=_Traced())
    ds.Optimize(8, 1e-4)
    assert ds.path.ctx.info("MODE") == api.MODE_SCHUR
    ds.path.close()
    print(name, "steps kept:", ds.path.trace, "chi2:", ["%.9g" % c for c in ds.chi2_history])
    assert ds.path.trace == hs.path.trace and ds.n_iterations == hs.n_iterations and len(ds.path.trace) >= 2
    assert hs.chi2_history[-1] < 0.05 * hs.chi2_history[0]
    for a, b in zip(dev.state(), host.state()):
        d = np.abs(a - b).max()
        print(name, "max state difference to the host loop: %.3e" % d)
        assert d <= 1e-6 * max(1.0, np.abs(b).max())
    assert abs(dev.chi2() - host.chi2()) <= 1e-9 * host.chi2()
    assert abs(ds.chi2_history[-1] - hs.chi2_history[-1]) <= 1e-9 * hs.chi2_history[-1]


def test_unmodified_slam_plus_plus_app_on_stereo_data_matches_the_reference_binary():
    """the reference's slam_plus_plus (sources untouched, SolveBAStereoImpl.cpp) on the golden's file, once with the HIP
    solver shimmed in and once as it is: the chi2 values printed agree to the printed digits, solution.txt as
    tests/test_gpu_dropin.py compares it for its BA case."""
    exe = {w: os.path.join(ROOT, "oracle", "_ref", "slam_plus_plus_" + w) for w in ("hip", "ref")}
    if not all(os.path.exists(e) for e in exe.values()):
        pytest.skip("oracle/_ref/slam_plus_plus_{hip,ref} not built (make -C oracle apps)")
    lines = np.load(GOLD)["lines"].tolist()
    res = {}
    with tempfile.TemporaryDirectory() as gdir:
        path = os.path.join(gdir, "stereo.txt")
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
        for w in ("hip", "ref"):
            with tempfile.TemporaryDirectory() as tmp:
                p = subprocess.run([exe[w], "-i", path, "-nb", "-ns"], cwd=tmp, env=dict(os.environ, OMP_NUM_THREADS="1"),
                                   capture_output=True, text=True, timeout=120)
                assert p.returncode == 0, (w, p.stdout[-1500:], p.stderr[-1500:])
                res[w] = (p.stdout, np.array(open(os.path.join(tmp, "solution.txt")).read().split(), dtype=np.float64))
    assert "Cholesky failed" not in res["hip"][0]
    chi = {w: re.findall(r"denormalized chi2 error: ([-+0-9.eE]+)", res[w][0]) for w in res}
    its = {w: re.findall(r"solver took (\d+) iterations", res[w][0]) for w in res}
    print(chi, its)
    assert len(chi["ref"]) == 2 and chi["hip"] == chi["ref"] and its["hip"] == its["ref"]
    a, b = res["hip"][1], res["ref"][1]
    assert a.size == b.size and a.size > 0
    assert np.all(np.abs(a - b) <= 2e-5 * np.abs(b) + 2e-6), np.abs(a - b).max()
