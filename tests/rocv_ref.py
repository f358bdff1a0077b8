"""Shared pieces of the range-only constant-velocity (ROCV) tests (no test functions; no GPU): the two edge models at 50
digits (mpmath; Jacobians by central differences at h = 1e-20, as tests/geometry_ref.py takes them), their edge cases, the
scales and the constant C of the bound |mirror or kernel - reference| <= C eps scale, a dense float64 Lambda of any list of
edge groups (binary and unary) and the numpy Gauss-Newton loop.

Models, from their definitions (reference include/slam/ROCV_Types.h):
  range  (CEdgePosVel_Landmark3D<false>, :163-205)   e = |p - l|, r = z - e, J0 = d e / d (p, v), J1 = d e / d l; at e = 0 the
         central difference of |.| is 0: both Jacobians zero, r = z -- what the kernel documents there
  cv     (CEdgeConstVelocity3D<false>, :543-614)     h(x0, x1) = x1 - (p0 + v0 dt, v0); the edge's error is r = -h (the reversed
         sign of :608) while its Jacobians are those of h: J0 = d h / d x0 = -[I, dt I; 0, I], J1 = d h / d x1 = I. Here
         J0 := -d r / d x0 and J1 := -d r / d x1 by central differences of r."""
import functools

import numpy as np

EPS = np.finfo(np.float64).eps
# per output: 8 x the largest quotient |mirror - reference| / (eps scale) over the cases (a quotient below 1 counts as 1),
# rounded up to a power of two (DESIGN section 18's rule); tests/test_rocv_host.py recomputes the quotients and fails if a
# constant here is not that
C = {"rng_J0": 8, "rng_J1": 8, "rng_r": 8, "cv_J0": 8, "cv_J1": 8, "cv_r": 8}


def range_cases():
    """p (k, 6) receivers, l (k, 3) transmitters, z (k,): generic edges; e = 0 (r = z, zero Jacobians); e = 1e-12; e = 1e6;
    receiver and transmitter coinciding in two coordinates; a negative and a zero measurement"""
    rng = np.random.default_rng(811)
    p = np.concatenate([rng.normal(0, 10, size=(8, 3)), rng.normal(0, 2, size=(8, 3))], axis=1)
    l = rng.normal(0, 10, size=(8, 3))
    z = np.abs(rng.normal(10, 5, size=8))
    l[1] = p[1, :3]                                            # e = 0
    l[2] = p[2, :3] + 1e-12 * np.array([0.6, 0.0, -0.8])       # e = 1e-12
    l[3] = p[3, :3] + 1e6 * np.array([2.0, -1.0, 2.0]) / 3.0   # e = 1e6
    l[4] = p[4, :3] + np.array([0.0, 0.0, 3.0])                # two coordinates coincide
    l[5] = p[5, :3] + np.array([0.0, -2.5, 0.0])
    z[6], z[7] = -1.5, 0.0
    return p, l, z


def cv_cases():
    """x0, x1 (m, 6) receivers, dt (m,): generic steps; dt = 0; dt < 0; a large state with a small step; x1 at the
    expectation (r = 0 up to rounding)"""
    rng = np.random.default_rng(812)
    x0 = np.concatenate([rng.normal(0, 10, size=(7, 3)), rng.normal(0, 2, size=(7, 3))], axis=1)
    dt = rng.uniform(0.1, 2.0, size=7)
    dt[1], dt[2], dt[3] = 0.0, -0.7, 1e-3
    x0[3] *= 1e4
    x1 = np.concatenate([x0[:, :3] + x0[:, 3:] * dt[:, None], x0[:, 3:]], axis=1) + rng.normal(0, 0.3, size=(7, 6))
    x1[4] = np.concatenate([x0[4, :3] + x0[4, 3:] * dt[4], x0[4, 3:]])
    return x0, x1, dt


@functools.lru_cache(maxsize=None)
def reference():
    """the 50-digit reference of both models on the cases, rounded once to float64: a dict of rng_J0 (k, 6), rng_J1 (k, 3),
    rng_r (k,), cv_J0 (m, 6, 6), cv_J1 (m, 6, 6), cv_r (m, 6)"""
    import mpmath as mp
    mp.mp.dps = 50
    h = mp.mpf(10) ** -20
    f64 = lambda v: float(v)

    def dist(x):   # x: p (6) then l (3)
        return mp.sqrt(sum((x[i] - x[6 + i]) ** 2 for i in range(3)))

    p, l, z = range_cases()
    out = {k: [] for k in ("rng_J0", "rng_J1", "rng_r")}
    for e in range(z.size):
        x = [mp.mpf(float(v)) for v in np.concatenate([p[e], l[e]])]
        J = []
        for c in range(9):
            xp, xm = list(x), list(x)
            xp[c] += h
            xm[c] -= h
            J.append(f64((dist(xp) - dist(xm)) / (2 * h)))
        out["rng_J0"].append(J[:6])
        out["rng_J1"].append(J[6:])
        out["rng_r"].append(f64(mp.mpf(float(z[e])) - dist(x)))

    def cv_r(x, dt):   # x: x0 (6) then x1 (6); the reference's error -(x1 - expectation)
        return [-(x[6 + i] - (x[i] + x[3 + i] * dt)) for i in range(3)] + [-(x[9 + i] - x[3 + i]) for i in range(3)]

    x0, x1, dts = cv_cases()
    out.update({k: [] for k in ("cv_J0", "cv_J1", "cv_r")})
    for e in range(dts.size):
        x = [mp.mpf(float(v)) for v in np.concatenate([x0[e], x1[e]])]
        dt = mp.mpf(float(dts[e]))
        J = np.empty((6, 12))
        for c in range(12):
            xp, xm = list(x), list(x)
            xp[c] += h
            xm[c] -= h
            rp, rm = cv_r(xp, dt), cv_r(xm, dt)
            J[:, c] = [f64(-(rp[i] - rm[i]) / (2 * h)) for i in range(6)]   # the Jacobians are those of -r
        out["cv_J0"].append(J[:, :6])
        out["cv_J1"].append(J[:, 6:])
        out["cv_r"].append([f64(v) for v in cv_r(x, dt)])
    return {k: np.array(v) for k, v in out.items()}


def scales():
    """scale of every output entry, from the inputs. Range: the unit vector's entries are quotients of correctly rounded
    differences and a norm of relative error a few eps -- scale 1; r: |z| + e. Constant velocity: r_i is a sum of x1_i, p0_i
    and v0_i dt (position rows) or v1_i, v0_i (velocity rows) -- the sum of their magnitudes (at least the smallest normal
    number, so that an exact zero compares); J0: 1 and |dt| (the entries are exact), J1: 1."""
    p, l, z = range_cases()
    e = np.linalg.norm(p[:, :3] - l, axis=1)
    x0, x1, dt = cv_cases()
    s_r = np.concatenate([np.abs(x1[:, :3]) + np.abs(x0[:, :3]) + np.abs(x0[:, 3:] * dt[:, None]),
                          np.abs(x1[:, 3:]) + np.abs(x0[:, 3:])], axis=1)
    s_J0 = np.ones((dt.size, 6, 6))
    s_J0[:, np.arange(3), 3 + np.arange(3)] = np.maximum(np.abs(dt), 1.0)[:, None]
    return {"rng_J0": np.ones((z.size, 6)), "rng_J1": np.ones((z.size, 3)), "rng_r": np.abs(z) + e,
            "cv_J0": s_J0, "cv_J1": np.ones((dt.size, 6, 6)), "cv_r": np.maximum(s_r, np.finfo(np.float64).tiny)}


def quotients(got):
    """largest |got - reference| / (eps scale) per output; got: a dict shaped like reference()"""
    ref, sc = reference(), scales()
    return {k: float((np.abs(np.asarray(got[k]).reshape(ref[k].shape) - ref[k]) / (EPS * sc[k])).max()) for k in ref}


def cases_as_state():
    """the cases laid out as ONE flat state addressed by scalar offsets, receivers and transmitters alternating (so that
    offsets are no multiple of a vertex width): state, (rng_off0, rng_off1, z), (cv_off0, cv_off1, dt)"""
    p, l, z = range_cases()
    x0, x1, dt = cv_cases()
    parts, off, pos = [], {}, 0
    for name, rows in (("p", p), ("l", l), ("x0", x0), ("x1", x1)):
        off[name] = []
    for i in range(max(z.size, dt.size)):
        for name, rows in (("l", l), ("p", p), ("x1", x1), ("x0", x0)):
            if i < rows.shape[0]:
                off[name].append(pos)
                parts.append(rows[i])
                pos += rows.shape[1]
    o = lambda name: np.array(off[name], dtype=np.int64)
    return np.concatenate(parts), (o("p"), o("l"), z), (o("x0"), o("x1"), dt)


def dense_lambda(groups, damping=0.0):
    """Lambda and eta of edge groups (synth.Problems over the same vertices; a group with v1 None is unary) in dense float64,
    every term J^T Omega J / J^T Omega r of the mirror summed edge by edge, + the unit unary factor when unary_vertex >= 0"""
    dim = np.asarray(groups[0].dim, dtype=np.int64)
    base = np.concatenate([[0], np.cumsum(dim)])
    n = int(base[-1])
    L, eta = np.zeros((n, n)), np.zeros(n)
    for g in groups:
        J0 = np.asarray(g.J0).reshape(-1, g.d0, g.rd).transpose(0, 2, 1)
        Om = np.asarray(g.Om).reshape(-1, g.rd, g.rd)
        r = np.asarray(g.r).reshape(-1, g.rd)
        w = np.ones(len(J0)) if g.get("w") is None else np.asarray(g["w"])
        unary = g.v1 is None
        J1 = None if unary else np.asarray(g.J1).reshape(-1, g.d1, g.rd).transpose(0, 2, 1)
        for e in range(len(J0)):
            sa = slice(base[g.v0[e]], base[g.v0[e]] + g.d0)
            A = J0[e].T @ Om[e]
            L[sa, sa] += A @ J0[e] * w[e]
            if unary:   # BaseTypes_Unary.h:560-569: the weight once on H and once on g
                eta[sa] += A @ r[e] * w[e]
                continue
            sb = slice(base[g.v1[e]], base[g.v1[e]] + g.d1)
            B = J1[e].T @ Om[e]
            L[sb, sb] += B @ J1[e] * w[e]
            L[sa, sb] += A @ J1[e] * w[e]
            L[sb, sa] += B @ J0[e] * w[e]
            eta[sa] += A @ r[e] * w[e] * w[e]   # BaseTypes_Binary.h:768-848: the first vertex's rhs carries w twice
            eta[sb] += B @ r[e] * w[e]
    u = groups[0].unary_vertex
    if u is not None and u >= 0:
        L[base[u]:base[u + 1], base[u]:base[u + 1]] += np.eye(int(dim[u]))
    L[np.arange(n), np.arange(n)] += damping
    return L, eta


class DensePath:
    @staticmethod
    def solve(groups, first):
        L, eta = dense_lambda(groups)
        return True, np.linalg.solve(L, eta)


def host_loop(system, max_iter=5, threshold=0.01):
    """the numpy Gauss-Newton loop, one Optimize(1) per iteration so that chi2 can be read in between.
    Returns (iterations, residual norms, chi2 before and after every applied step)."""
    from slam_plus_plus_amd import nonlinear
    norms, chi2 = [], [system.chi2()]
    for it in range(max_iter):
        solver = nonlinear.CNonlinearSolver_Lambda(system, path=DensePath())
        solver.Optimize(1, threshold)
        norms.append(solver.last_dx_norm)
        if solver.last_dx_norm <= threshold:
            break
        chi2.append(system.chi2())
    return len(norms), norms, chi2


@functools.lru_cache(maxsize=None)
def host_result(name):
    """(final state, iterations, norms) of the numpy loop on a synth fixture: computed once, shared by the tests"""
    from slam_plus_plus_amd import nonlinear, synth
    s = nonlinear.CRocv.from_problem(synth.make(name))
    n_it, norms, _ = host_loop(s)
    s.state.setflags(write=False)
    return s.state, n_it, norms
