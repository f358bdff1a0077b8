"""3D landmark SLAM on the device: the offset-addressed SE(3) odometry kernel, the XYZ observation kernel
(CEdgePoseLandmark3D), the flat-state update and the resident Gauss-Newton loop over the groups (6,6,6) + (6,3,3), against
the numpy mirror (formats.slam3d_linearize, nonlinear.CSlam3D with a dense float64 solve)."""
import functools

import numpy as np
import pytest

from slam_plus_plus_amd import api, nonlinear, synth
from slam_plus_plus_amd.formats import slam3d_linearize, slam3d_offsets
from test_slam3d_host import edge_case_state, host_loop

pytestmark = pytest.mark.gpu
FIXTURES = ["slam3d_small", "slam3d_interleaved"]


@functools.lru_cache(maxsize=None)
def _host_run(name):
    """the numpy loop, once per fixture: (iterations, final state, chi2 before and after every applied step)"""
    s = nonlinear.CSlam3D.from_problem(synth.make(name))
    n_it, _, chi = host_loop(s)
    return n_it, s.state.copy(), chi


def _relmax(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def test_offsets_of_6_id_reproduce_the_id_addressed_kernel():
    prob = synth.make("se3_small")
    st = synth.pose_graph_states(prob)
    ne = st["v0"].size
    ctx = api.Context(0)
    up = lambda a: api.DeviceArray.from_host(ctx, np.ascontiguousarray(a).ravel())
    poses, meas = up(st["poses"]), up(st["meas"])
    a = [api.DeviceArray(ctx, n * ne) for n in (36, 36, 6)]
    b = [api.DeviceArray(ctx, n * ne) for n in (36, 36, 6)]
    ctx.se3_linearize_device(ne, up(st["v0"]).ptr, up(st["v1"]).ptr, poses.ptr, meas.ptr, *[x.ptr for x in a])
    ctx.se3_linearize_at_device(ne, up(6 * st["v0"].astype(np.int64)).ptr, up(6 * st["v1"].astype(np.int64)).ptr, poses.ptr,
                                meas.ptr, *[x.ptr for x in b])
    ctx.synchronize()
    for x, y in zip(a, b):
        assert np.abs(x.download()).max() > 0 and np.array_equal(x.download(), y.download())
    ctx.close()


def test_xyz_linearize_kernel_matches_the_numpy_mirror():
    p = synth.make("slam3d_interleaved")
    x, (k0, k1, k2) = edge_case_state(p)
    base = slam3d_offsets(p.dim)
    g_odo, g_obs = slam3d_linearize(p.dim, x, p.odo, p.odo_info, p.obs, p.obs_info)
    # the inputs do hold the cases: small-angle branch, a rotation next to pi, a landmark at its pose
    ang = np.linalg.norm(x[base[g_obs.v0][:, None] + 3 + np.arange(3)], axis=1)
    assert ang[k0] < 1e-10 and abs(ang[k1] - np.pi) < 1e-3
    assert np.array_equal(x[base[g_obs.v1[k2]]:][:3], x[base[g_obs.v0[k2]]:][:3]) and np.array_equal(g_obs.r[k2], p.obs[k2, 2:5])
    assert (g_obs.v1 < g_obs.v0).any() and (g_obs.v1 > g_obs.v0).any()
    ctx = api.Context(0)
    up = lambda a: api.DeviceArray.from_host(ctx, np.ascontiguousarray(a).ravel())
    d_state = up(x)
    m, k = p.odo.shape[0], p.obs.shape[0]
    out = [api.DeviceArray(ctx, n) for n in (36 * m, 36 * m, 6 * m, 18 * k, 9 * k, 3 * k)]
    ctx.se3_linearize_at_device(m, up(base[g_odo.v0]).ptr, up(base[g_odo.v1]).ptr, d_state.ptr, up(p.odo[:, 2:8]).ptr,
                                out[0].ptr, out[1].ptr, out[2].ptr)
    ctx.se3_xyz_linearize_device(k, up(base[g_obs.v0]).ptr, up(base[g_obs.v1]).ptr, d_state.ptr, up(p.obs[:, 2:5]).ptr,
                                 out[3].ptr, out[4].ptr, out[5].ptr)
    ctx.synchronize()
    errs = [_relmax(o.download(), w.ravel()) for o, w in zip(out[3:], (g_obs.J0, g_obs.J1, g_obs.r))]
    print("relative max-abs differences (observation J0 J1 r):", ["%.2e" % e for e in errs])
    assert max(errs) <= 1e-12, errs
    got = [o.download().reshape(k, -1) for o in out[3:]]
    for kc in (k0, k1, k2):     # the cases themselves, against entries of order 1 (-I in J0, R^T in J1, the measurement)
        for o, w in zip(got, (g_obs.J0, g_obs.J1, g_obs.r)):
            assert np.abs(o[kc] - w[kc]).max() <= 1e-12 * max(1.0, np.abs(w[kc]).max()), kc
    # the odometry through offsets, at the same state: the bound the se3 geometry meets against its goldens
    errs = [_relmax(o.download(), w.ravel()) for o, w in zip(out[:3], (g_odo.J0, g_odo.J1, g_odo.r))]
    print("relative max-abs differences (odometry J0 J1 r):", ["%.2e" % e for e in errs])
    assert max(errs) <= 1e-12, errs
    ctx.close()


def test_update_composes_poses_and_adds_landmarks():
    s = nonlinear.CSlam3D.from_problem(synth.make("slam3d_interleaved"))
    rng = np.random.default_rng(9)
    x = s.state.copy()
    dx = rng.normal(size=x.size) * 0.3
    pose_idx = s.pose_off[:, None] + np.arange(6)
    lm = np.setdiff1d(np.arange(x.size), pose_idx.ravel())
    ctx = api.Context(0)
    d_x, d_dx = api.DeviceArray.from_host(ctx, x), api.DeviceArray.from_host(ctx, dx)
    d_p = api.DeviceArray.from_host(ctx, s.pose_off.astype(np.int64))
    norm = ctx.slam3d_update_device(x.size, d_x.ptr, d_dx.ptr, s.pose_off.size, d_p.ptr, apply=False)
    assert abs(norm - np.linalg.norm(dx)) <= 1e-14 * np.linalg.norm(dx)
    assert np.array_equal(d_x.download(), x)            # apply=False: untouched
    assert ctx.slam3d_update_device(x.size, d_x.ptr, d_dx.ptr, s.pose_off.size, d_p.ptr, apply=True) == norm
    got = d_x.download()
    assert np.array_equal(got[lm], (x + dx)[lm])        # landmarks: plain sums, bit for bit
    # poses: the composition spp_se3_update_device applies to the same poses and increments, bit for bit
    d_poses, d_inc = api.DeviceArray.from_host(ctx, x[pose_idx].ravel()), api.DeviceArray.from_host(ctx, dx[pose_idx].ravel())
    ctx.se3_update_device(s.pose_off.size, d_poses.ptr, d_inc.ptr, apply=True)
    assert np.array_equal(got[pose_idx].ravel(), d_poses.download())
    assert not np.array_equal(got[pose_idx], (x + dx)[pose_idx])                 # (a composition, not a sum)
    s.plus(dx)
    assert np.abs(got - s.state).max() <= 1e-12 * np.abs(s.state).max()          # and the numpy (+)
    ctx.close()


def _check_state(state, name):
    """the bound tests/test_nonlinear_gn.py:57-58 (_check) applies to the device-vs-host comparison of the se2 loop"""
    _, final, _ = _host_run(name)
    d = np.abs(state - final).max()
    print(name, "max state difference to the numpy loop: %.3e" % d)
    assert d <= 1e-6 * max(1.0, np.abs(final).max()), d


@pytest.mark.parametrize("name", FIXTURES)
def test_resident_gauss_newton_matches_the_numpy_loop(name):
    n_host, _, chi_host = _host_run(name)
    assert all(b <= a for a, b in zip(chi_host, chi_host[1:])) and chi_host[-1] < 0.01 * chi_host[0]   # the fixture itself
    s = nonlinear.CSlam3D.from_problem(synth.make(name))
    solver = nonlinear.CNonlinearSolver_Lambda(s)
    assert isinstance(solver.path, nonlinear._ResidentSlam3DPath)
    assert solver.Optimize(5, 0.01) == n_host
    assert solver.path.ctx.info("MODE") == api.MODE_SCHUR
    _check_state(s.state, name)
    solver.path.close()
    # chi2 along the way, on the device: the same protocol driven by hand
    path = nonlinear._ResidentSlam3DPath()
    path.begin(nonlinear.CSlam3D.from_problem(synth.make(name)))
    chi = [path.chi2()]
    for _ in range(5):
        ok, norm = path.step()
        assert ok
        if norm <= 0.01:
            break
        path.apply()
        chi.append(path.chi2())
    path.close()
    print(name, "chi2:", ["%.6g" % c for c in chi])
    assert len(chi) == len(chi_host) and all(b <= a for a, b in zip(chi, chi[1:])) and chi[-1] < 0.01 * chi[0]
    assert abs(chi[0] - chi_host[0]) <= 1e-9 * chi_host[0] and abs(chi[-1] - chi_host[-1]) <= 1e-6 * chi_host[-1]


@pytest.mark.parametrize("name", FIXTURES)
def test_host_jacobian_path_reaches_the_same_state(name):
    n_host, _, _ = _host_run(name)
    s = nonlinear.CSlam3D.from_problem(synth.make(name))
    solver = nonlinear.CNonlinearSolver_Lambda(s, host_jacobians=True)
    assert isinstance(solver.path, nonlinear._DeviceGroupsPath)
    assert solver.Optimize(5, 0.01) == n_host
    _check_state(s.state, name)
    solver.path.close()
