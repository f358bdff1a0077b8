"""Shared pieces of the self-calibrating bundle adjustment tests (no test functions; no GPU): the padded float64 Lambda of
a bai_linearize Problem as a sparse matrix, the Levenberg-Marquardt path on the host, the fixtures, and the constant C of
the geometry bound |mirror - reference| <= C eps scale (tests/bai_ref.py states the scales, test_bai_host.py recomputes C)."""
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from slam_plus_plus_amd import nonlinear, synth

FIXTURES = ["bai_tiny", "bai_small", "bai_hub"]
EPS = np.finfo(np.float64).eps
# per output: 8 x the largest quotient |mirror - reference| / (eps scale) over edge_cases() (a quotient below 1 counts as 1),
# rounded up to a power of two (DESIGN section 18's rule); tests/test_bai_host.py recomputes the quotients and fails if a
# constant here is not that
C = {"J0": 8, "J1": 8, "J2": 8, "r": 8}


@functools.lru_cache(maxsize=None)
def fixture(name, layout="first"):
    return getattr(synth, name)(layout)


def padded_lambda(prob, damping=0.0):
    """(Lambda csc (n, n), eta (n)) of a bai_linearize Problem in the padded layout, float64: J^T Omega J over the three
    vertices of every edge, the unary factor (identity on the live coordinates), the damping on every diagonal entry, 1.0
    on the inert diagonal entries. The sparse twin of formats.bai_assemble_dense."""
    dim = np.asarray(prob.dim, dtype=np.int64)
    base = np.concatenate([[0], np.cumsum(dim)])
    n, no = int(base[-1]), prob.v0.size
    Om = prob.Om.reshape(no, 2, 2)
    Js = [(np.asarray(prob.v0), prob.J0.reshape(no, 6, 2).transpose(0, 2, 1)),
          (np.asarray(prob.v1), prob.J1.reshape(no, 3, 2).transpose(0, 2, 1)),
          (np.asarray(prob.v2), prob.J2.reshape(no, 6, 2).transpose(0, 2, 1))]
    rows, cols, vals = [], [], []
    eta = np.zeros(n)
    for va, Ja in Js:
        wa = Ja.shape[2]
        ia = base[va][:, None] + np.arange(wa)
        np.add.at(eta, ia, np.einsum("eli,elm,em->ei", Ja, Om, prob.r))
        for vb, Jb in Js:
            wb = Jb.shape[2]
            H = np.einsum("eli,elm,emj->eij", Ja, Om, Jb)
            ib = base[vb][:, None] + np.arange(wb)
            rows.append(np.broadcast_to(ia[:, :, None], H.shape).ravel())
            cols.append(np.broadcast_to(ib[:, None, :], H.shape).ravel())
            vals.append(H.ravel())
    diag = np.full(n, float(damping))
    is_intr = np.zeros(dim.size, dtype=bool)
    is_intr[prob.v2] = True
    u = prob.unary_vertex
    if u is not None and u >= 0:
        diag[base[u] + np.arange(5 if is_intr[u] else int(dim[u]))] += 1.0
    diag[base[:-1][is_intr] + 5] += 1.0
    rows.append(np.arange(n)); cols.append(np.arange(n)); vals.append(diag)
    lam = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsc()
    return lam, eta


def solve_padded(lam, eta, dim):
    """float64 solve of the padded system: dense LAPACK up to 2000 unknowns; beyond, sparse LU (SuperLU) in the order
    points first, then the 6-wide vertices -- the fill then stays inside the reduced camera system"""
    if lam.shape[0] <= 2000:
        return np.linalg.solve(lam.toarray(), eta)
    width = np.repeat(np.asarray(dim), np.asarray(dim))
    perm = np.argsort(width, kind="stable")
    lu = spla.splu(lam[perm][:, perm].tocsc(), permc_spec="NATURAL", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
    x = np.empty_like(eta)
    x[perm] = lu.solve(eta[perm])
    return x


class HostBAIPath:
    """the LM path on the host: numpy linearization (the mirror), float64 Lambda and solve in the padded layout"""

    def begin(self, s):
        self.s = s
        self.trace = []     # True per accepted step, False per rejected one

    def linearize(self):
        self.prob = self.s.linearize()

    def max_hessian_diag(self):
        p = self.prob
        Om = p.Om.reshape(-1, 2, 2)
        return max(np.einsum("eci,eij,ecj->ec", J.reshape(-1, d, 2), Om, J.reshape(-1, d, 2)).max()
                   for J, d in ((p.J0, 6), (p.J1, 3), (p.J2, 6)))

    def chi2(self):
        self.linearize()
        return float(np.einsum("ei,eij,ej->", self.prob.r, self.prob.Om.reshape(-1, 2, 2), self.prob.r))

    def solve(self, alpha):
        lam, eta = padded_lambda(self.prob, alpha)
        self.dx, self.eta = solve_padded(lam, eta, self.prob.dim), eta
        return True, float(np.linalg.norm(self.dx))

    def gain_denominator(self, alpha):
        return float(self.dx @ (alpha * self.dx + self.eta))

    def save(self):
        self.saved = self.s.state()
        self.trace.append(True)

    def restore(self):
        self.s.set_state(self.saved)
        self.trace[-1] = False

    def apply(self):
        self.s.plus(self.dx)

    def finish(self, s):
        pass


def host_lm(name, iters=5, threshold=0.01):
    s = nonlinear.CBundleAdjustmentIntrinsics.from_problem(fixture(name))
    solver = nonlinear.CNonlinearSolver_Lambda_LM(s, path=HostBAIPath())
    solver.Optimize(iters, threshold)
    return s, solver


# ----------------------------------------------------------------------------------------------------------------------
# the 50-digit cases of the ternary edge (tests/bai_ref.py; tools/make_golden_bai_edges.py -> tests/golden/bai_edges.npz)
# ----------------------------------------------------------------------------------------------------------------------
def edge_cases():
    """The mono BA cases of geometry_cases.ba_cases() -- every cell of the camera's angle (0, 2e-7, generic, beyond pi),
    kappa = 0, r2 k = 0.3, a point on the axis, one behind the camera, |X| = 1e3, fx != fy throughout -- with one intrinsics
    VERTEX per row of its intr: cams (nc, 6), intr (ni, 5), pts (np, 3), obs (no, 5) cam pt intr u v. An observation uses the
    intrinsics vertex of its camera; the gather observations at the end use those of OTHER cameras (ids reversed: an
    intrinsics index above and below the camera's) and one vertex repeatedly."""
    import geometry_cases as gc
    cams, intr, pts, obs = gc.ba_cases()
    io = obs[:, 0].copy()
    rep = np.flatnonzero((obs[:, 0] != obs[:, 1]))     # the gathers: camera c sees the point of another camera's case
    io[rep] = obs[rep, 1]                              # ... through that camera's intrinsics vertex
    io[rep[:2]] = 3.0                                  # ... and two of them through vertex 3
    return cams, intr, pts, np.concatenate([obs[:, :2], io[:, None], obs[:, 2:4]], axis=1)


def edge_scales(cams, intr, pts, obs, aux):
    """scale of every output entry in |mirror - reference| <= C eps scale. J0, J1, r: the projection scales of DESIGN
    section 18 (geometry_cases._proj_scales, with the intrinsics the observation uses). J2, from the inputs: with rho =
    (|R||X| + |t|) / |z| >= 1 the conditioning of x / z, f = fx + fy, amp = 1 + 3 (f rho)^2 |k| the distortion's
    amplification, per unit of fx or fy: amp rho^2 (uv / f); per unit of cx, cy: 1 (the entries are exact); per unit of
    kappa: r^2 |p - c| / (0.5 f) with |p - c| <= f rho; the inert column: 0 (exact zeros)."""
    import geometry_cases as gc
    co, io = obs[:, 0].astype(int), obs[:, 2].astype(int)
    # _proj_scales indexes intr by the camera: give it one row per OBSERVATION instead
    k = obs.shape[0]
    g = {"ba_cams": cams[co], "ba_intr": intr[io], "ba_pts": pts[obs[:, 1].astype(int)],
         "ba_obs": np.concatenate([np.arange(k)[:, None], np.arange(k)[:, None], obs[:, 3:5]], axis=1), "ba_aux": aux}
    s = gc._proj_scales(g, "ba", False)
    c, X, it = g["ba_cams"], g["ba_pts"], g["ba_intr"]
    th = 1 + np.linalg.norm(c[:, 3:], axis=1)
    rho = (th * np.linalg.norm(X, axis=1) + np.linalg.norm(c[:, :3], axis=1)) / np.abs(aux[:, 2])
    f = it[:, 0] + it[:, 1]
    amp = 1 + 3 * (f * rho) ** 2 * np.abs(it[:, 4]) / (0.5 * f)
    s_f, s_k, one, zero = amp * rho * rho, (f * rho) ** 3 / (0.5 * f), np.ones(k), np.zeros(k)
    s["J2"] = np.stack([s_f, s_f, s_f, s_f, one, one, one, one, s_k, s_k, zero, zero], axis=1)
    return s
