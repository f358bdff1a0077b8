"""2D landmark SLAM on the device: the offset-addressed odometry kernel, the range-bearing kernel
(CEdgePoseLandmark2D), the flat-state update and the resident Gauss-Newton loop over two edge groups, against the numpy
mirror (formats.slam2d_linearize, nonlinear.CSlam2D with a dense float64 solve)."""
import functools

import numpy as np
import pytest

from slam_plus_plus_amd import api, nonlinear, synth
from slam_plus_plus_amd.formats import slam2d_linearize

pytestmark = pytest.mark.gpu
FIXTURES = ["slam2d_small", "slam2d_interleaved"]


class _DensePath:
    """Lambda and eta of all groups in dense float64, numpy solve: the host side of every comparison here"""

    def solve(self, groups, first):
        dim = groups[0].dim
        base = np.zeros(dim.size + 1, dtype=np.int64)
        np.cumsum(dim, out=base[1:])
        n = int(base[-1])
        L, eta = np.zeros((n, n)), np.zeros(n)
        for g in groups:
            J0 = g.J0.reshape(-1, g.d0, g.rd).transpose(0, 2, 1)
            J1 = g.J1.reshape(-1, g.d1, g.rd).transpose(0, 2, 1)
            Om = g.Om.reshape(-1, g.rd, g.rd)
            for e in range(g.v0.size):
                sa, sb = slice(base[g.v0[e]], base[g.v0[e]] + g.d0), slice(base[g.v1[e]], base[g.v1[e]] + g.d1)
                A, B = J0[e].T @ Om[e], J1[e].T @ Om[e]
                L[sa, sa] += A @ J0[e]
                L[sb, sb] += B @ J1[e]
                L[sa, sb] += A @ J1[e]
                L[sb, sa] += B @ J0[e]
                eta[sa] += A @ g.r[e]
                eta[sb] += B @ g.r[e]
        u = groups[0].unary_vertex
        L[base[u]:base[u + 1], base[u]:base[u + 1]] += np.eye(dim[u])
        return True, np.linalg.solve(L, eta)


@functools.lru_cache(maxsize=None)
def _host_run(name):
    """the numpy loop, once per fixture: (iterations, final state, chi2 before and after every applied step)"""
    s = nonlinear.CSlam2D.from_problem(synth.make(name))
    chi = [s.chi2()]
    total = 0
    for _ in range(5):                       # one iteration at a time, to record chi2 in between
        solver = nonlinear.CNonlinearSolver_Lambda(s, path=_DensePath())
        solver.Optimize(1, 0.01)
        total += 1
        if solver.last_dx_norm <= 0.01:
            break
        chi.append(s.chi2())
    return total, s.state.copy(), chi


def _relmax(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def _edge_cases(name):
    """the fixture's graph at a state that holds: an observation at range below the 1e-5 floor, bearings within 1e-3 of
    +pi and of -pi with the measurement on the other side of the cut (wrap of the expectation and of the error), pose
    headings beyond +-2 pi"""
    p = synth.make(name)
    s = nonlinear.CSlam2D.from_problem(p)
    x, obs = s.state, s.obs.copy()
    used_p, used_l, picks = set(), set(), []
    for k in range(obs.shape[0]):             # three observations that share neither pose nor landmark
        a, b = int(obs[k, 0]), int(obs[k, 1])
        if a not in used_p and b not in used_l:
            picks.append(k)
            used_p.add(a)
            used_l.add(b)
        if len(picks) == 3:
            break
    k0, k1, k2 = picks
    pb, lb = lambda k: s.base[int(obs[k, 0])], lambda k: s.base[int(obs[k, 1])]
    x[lb(k0):lb(k0) + 2] = x[pb(k0):pb(k0) + 2] + np.array([6e-7, -3e-7])
    for k, sign in ((k1, 1.0), (k2, -1.0)):
        d = x[lb(k):lb(k) + 2] - x[pb(k):pb(k) + 2]
        x[pb(k) + 2] = np.arctan2(d[1], d[0]) - sign * (np.pi - 5e-4)     # expectation 5e-4 inside +-pi
        obs[k, 3] = -sign * (np.pi - 4e-4)                                # measurement across the cut: error ~ -+9e-4 after the wrap
    far = s.angle_off[5::7]
    x[far] += 2 * np.pi * np.arange(1, far.size + 1) * np.where(np.arange(far.size) % 2, 1, -1)
    s.obs = obs
    return s, (k0, k1, k2)


def test_both_linearize_kernels_match_the_numpy_mirror():
    s, (k0, k1, k2) = _edge_cases("slam2d_interleaved")
    g_odo, g_obs = slam2d_linearize(s.dim, s.state, s.odo, s.odo_info, s.obs, s.obs_info)
    # the inputs do hold the cases
    d = s.state[s.base[g_obs.v1][:, None] + np.arange(2)] - s.state[s.base[g_obs.v0][:, None] + np.arange(2)]
    assert np.hypot(d[k0, 0], d[k0, 1]) < 1e-5 and abs(g_obs.r[k0, 0] - (s.obs[k0, 2] - 1e-5)) < 1e-15
    assert abs(abs(g_obs.r[k1, 1]) - 9e-4) < 1e-6 and abs(abs(g_obs.r[k2, 1]) - 9e-4) < 1e-6 and g_obs.r[k1, 1] * g_obs.r[k2, 1] < 0
    assert (g_obs.v1 < g_obs.v0).any() and np.abs(s.state[s.angle_off]).max() > 4 * np.pi
    ctx = api.Context(0)
    up = lambda a: api.DeviceArray.from_host(ctx, np.ascontiguousarray(a).ravel())
    d_state = up(s.state)
    m, k = s.odo.shape[0], s.obs.shape[0]
    out = [api.DeviceArray(ctx, n) for n in (9 * m, 9 * m, 3 * m, 6 * k, 4 * k, 2 * k)]
    ctx.se2_linearize_at_device(m, up(s.base[g_odo.v0]).ptr, up(s.base[g_odo.v1]).ptr, d_state.ptr, up(s.odo[:, 2:5]).ptr,
                                out[0].ptr, out[1].ptr, out[2].ptr)
    ctx.se2_rb_linearize_device(k, up(s.base[g_obs.v0]).ptr, up(s.base[g_obs.v1]).ptr, d_state.ptr, up(s.obs[:, 2:4]).ptr,
                                out[3].ptr, out[4].ptr, out[5].ptr)
    ctx.synchronize()
    want = (g_odo.J0, g_odo.J1, g_odo.r, g_obs.J0, g_obs.J1, g_obs.r)
    errs = [_relmax(o.download(), w.ravel()) for o, w in zip(out, want)]
    print("relative max-abs differences (odometry J0 J1 r, observation J0 J1 r):", ["%.2e" % e for e in errs])
    assert max(errs) <= 1e-13, errs
    # the floored observation puts entries of ~1e4 into the observation Jacobians and with them into the denominator:
    # the same bound over the other observations alone, whose entries are of order 1
    rest = np.arange(k) != k0
    errs = [_relmax(o.download().reshape(k, -1)[rest], w.reshape(k, -1)[rest]) for o, w in zip(out[3:], want[3:])]
    print("without the floored observation (observation J0 J1 r):", ["%.2e" % e for e in errs])
    assert max(errs) <= 1e-13, errs
    ctx.close()


def test_offsets_of_3_id_reproduce_the_id_addressed_kernel():
    prob = synth.make("se2_small")
    st = synth.pose_graph_states(prob)
    ne = st["v0"].size
    ctx = api.Context(0)
    up = lambda a: api.DeviceArray.from_host(ctx, np.ascontiguousarray(a).ravel())
    poses, meas = up(st["poses"]), up(st["meas"])
    a = [api.DeviceArray(ctx, n * ne) for n in (9, 9, 3)]
    b = [api.DeviceArray(ctx, n * ne) for n in (9, 9, 3)]
    ctx.se2_linearize_device(ne, up(st["v0"]).ptr, up(st["v1"]).ptr, poses.ptr, meas.ptr, *[x.ptr for x in a])
    ctx.se2_linearize_at_device(ne, up(3 * st["v0"].astype(np.int64)).ptr, up(3 * st["v1"].astype(np.int64)).ptr, poses.ptr,
                                meas.ptr, *[x.ptr for x in b])
    ctx.synchronize()
    for x, y in zip(a, b):
        assert np.array_equal(x.download(), y.download())
    ctx.close()


def test_update_clamps_pose_angles_only():
    s = nonlinear.CSlam2D.from_problem(synth.make("slam2d_interleaved"))
    rng = np.random.default_rng(9)
    x = s.state.copy()
    lm = np.setdiff1d(np.arange(x.size), np.concatenate([s.angle_off - 2, s.angle_off - 1, s.angle_off]))
    x[lm[:10]] += 40.0                                  # landmark coordinates far beyond 2 pi
    x[s.angle_off[:10]] += 5.0
    dx = rng.normal(size=x.size) * 3
    ctx = api.Context(0)
    d_x, d_dx = api.DeviceArray.from_host(ctx, x), api.DeviceArray.from_host(ctx, dx)
    d_a = api.DeviceArray.from_host(ctx, s.angle_off.astype(np.int64))
    norm = ctx.slam2d_update_device(x.size, d_x.ptr, d_dx.ptr, s.angle_off.size, d_a.ptr, apply=False)
    assert abs(norm - np.linalg.norm(dx)) <= 1e-14 * np.linalg.norm(dx)
    assert np.array_equal(d_x.download(), x)            # apply=False: untouched
    norm2 = ctx.slam2d_update_device(x.size, d_x.ptr, d_dx.ptr, s.angle_off.size, d_a.ptr, apply=True)
    assert norm2 == norm
    want = x + dx
    want[s.angle_off] = np.fmod(want[s.angle_off], 2 * np.pi)
    got = d_x.download()
    assert np.array_equal(got[lm], want[lm]) and got[lm].max() > 2 * np.pi      # landmarks: plain sums
    assert np.abs(got - want).max() <= 1e-14 and np.abs(got[s.angle_off]).max() < 2 * np.pi
    assert (np.abs((x + dx)[s.angle_off]) > 2 * np.pi).any()                    # (some angle did need the clamp)
    ctx.close()


def _check_state(state, name):
    """the bound tests/test_nonlinear_gn.py:57-58 (_check) applies to the device-vs-host comparison of the se2 loop"""
    _, final, _ = _host_run(name)
    d = np.abs(state - final).max()
    assert d <= 1e-6 * max(1.0, np.abs(final).max()), d


@pytest.mark.parametrize("name", FIXTURES)
def test_resident_gauss_newton_matches_the_numpy_loop(name):
    n_host, _, chi_host = _host_run(name)
    assert all(b <= a for a, b in zip(chi_host, chi_host[1:])) and chi_host[-1] < 0.01 * chi_host[0]   # the fixture itself
    s = nonlinear.CSlam2D.from_problem(synth.make(name))
    solver = nonlinear.CNonlinearSolver_Lambda(s)
    assert isinstance(solver.path, nonlinear._ResidentSlam2DPath)
    assert solver.Optimize(5, 0.01) == n_host
    assert solver.path.ctx.info("MODE") == api.MODE_SCHUR
    _check_state(s.state, name)
    solver.path.close()
    # chi2 along the way, on the device: the same protocol driven by hand
    path = nonlinear._ResidentSlam2DPath()
    path.begin(nonlinear.CSlam2D.from_problem(synth.make(name)))
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
    s = nonlinear.CSlam2D.from_problem(synth.make(name))
    solver = nonlinear.CNonlinearSolver_Lambda(s, host_jacobians=True)
    assert isinstance(solver.path, nonlinear._DeviceGroupsPath)
    assert solver.Optimize(5, 0.01) == n_host
    _check_state(s.state, name)
    solver.path.close()
