"""The cases, scales and constants of the Sim(3) geometry tests (no test functions; no GPU): tests/sim3_ref.py is the
50-digit reference, tools/make_golden_sim3_edges.py writes tests/golden/sim3_edges.npz from these cases, tests/test_sim3_host.py
pins the float64 mirror (formats.sim3_ba_linearize / sim3_plus) and the constants C, tests/test_gpu_sim3_geometry.py the
kernels -- DESIGN section 18's method."""
import numpy as np

from slam_plus_plus_amd import formats

EPS = np.finfo(np.float64).eps
AXES = np.array([[0.6, -0.48, 0.64], [0.0, 0.0, 1.0], [-0.36, 0.8, 0.48], [0.8, 0.6, 0.0]])
# |s| and |w|: zero, inside (0, 1e-12), within 1 % below and above the reference's 1e-6, generic
S_CELL = [0.0, 3e-13, -0.995e-6, 1.005e-6, 0.3]
W_CELL = [0.0, 3e-13, 0.995e-6, 1.005e-6, 0.7]
INTR = np.array([500.0, 480.0, 320.0, 240.0, 0.04 * 120000.0 / 2429.44])   # fx != fy; r^2 k = 0.04 at the generic point
XC = np.array([0.4, -0.3, 5.0])                                            # the generic camera-frame point: p - c = (40, -28.8)


def _cam(t, axis, th, s):
    return np.concatenate([np.asarray(t, dtype=np.float64), th * AXES[axis], [s]])


def _world(cam, xc):
    """the world point whose camera-frame image is (about) xc: sigma R xc + tau in float64 -- an input like any other"""
    R, tau, E, _ = formats.sim3_exp(cam[None])
    return E[0] * (R[0] @ np.asarray(xc, dtype=np.float64)) + tau[0]


def cell_cams():
    """one camera per cell of (|s|, |w|), then the cells of the kernel's own evaluation (Taylor series below s^2 + |w|^2 = 1,
    closed form beyond; two-term sinc below |w| = 1e-4) on both sides, |w| beyond pi, s = +-2"""
    cams = []
    for i, s in enumerate(S_CELL):
        for j, th in enumerate(W_CELL):
            cams.append(_cam([0.5 + 0.1 * i, -0.25 - 0.2 * j, 1.0 + 0.05 * (i - j)], (i + j) % 4, th, s))
    extra = [([1.0, 2.0, -0.5], 0, 0.79, 0.6), ([1.0, 2.0, -0.5], 0, 0.81, 0.6),        # s^2 + th^2 = 0.984, 1.016
             ([-0.3, 0.4, 0.2], 2, 0.99e-4, 1.2), ([-0.3, 0.4, 0.2], 2, 1.01e-4, 1.2),  # the sinc threshold, closed form
             ([-0.3, 0.4, 0.2], 3, 0.99e-4, 0.1), ([-0.3, 0.4, 0.2], 3, 1.01e-4, 0.1),  # ... and inside the series
             ([0.2, -0.1, 0.3], 1, 0.0, 1.0), ([0.2, -0.1, 0.3], 1, 1.0, 0.0),          # on the unit circle, either axis
             ([2.0, 1.0, -1.0], 0, 4.0, 0.3), ([2.0, 1.0, -1.0], 2, 5.5, 0.0), ([2.0, 1.0, -1.0], 3, 3.5, -1e-7),   # |w| in (pi, 2 pi)
             ([0.7, 0.1, 0.4], 1, 0.7, 2.0), ([0.7, 0.1, 0.4], 2, 0.7, -2.0), ([0.7, 0.1, 0.4], 0, 0.0, 2.0),
             ([0.7, 0.1, 0.4], 3, 2e-7, -2.0)]
    return np.array(cams + [_cam(*e) for e in extra])


def edge_cases():
    """cams (nc, 7), intr (nc, 5), pts (np, 3), obs (no, 4) cam pt u v: every camera of cell_cams() sees the generic point;
    then on the generic camera r^2 k = 0.3, kappa = 0, a point behind the camera, |X| = 1e3, and on the (0, 0) cell a point
    exactly on the optical axis; then gathers (a camera index above and below the point's)."""
    cams = cell_cams()
    nc0 = cams.shape[0]
    generic = 24                                                    # (s, |w|) = (0.3, 0.7)
    intr = np.tile(INTR, (nc0, 1))
    pts = [_world(c, XC) for c in cams]
    obs = [[i, i, 320 + 40.7 + 0.3 * i, 240 - 28.8 - 0.2 * i] for i in range(nc0)]

    def add(cam, it, X, z):
        nonlocal cams, intr
        cams = np.vstack([cams, cam[None]])
        intr = np.vstack([intr, np.asarray(it, dtype=np.float64)[None]])
        pts.append(np.asarray(X, dtype=np.float64))
        obs.append([cams.shape[0] - 1, len(pts) - 1, z[0], z[1]])

    g = cams[generic]
    add(g, [500, 480, 320, 240, 0.3 * 120000.0 / 2429.44], _world(g, XC), (380.0, 200.0))     # r^2 k = 0.3
    add(g, [500, 480, 320, 240, 0.0], _world(g, XC), (360.0, 211.0))                          # kappa = 0
    add(g, INTR, _world(g, [0.4, -0.3, -5.0]), (280.0, 270.0))                                # behind the camera
    add(g, [510, 470, 300, 250, INTR[4]], _world(g, np.array([60.0, -45.0, 995.0]) / np.exp(0.3)), (330.0, 229.0))    # |X| = 1e3
    axis_cam = np.array([0.5, -0.25, 1.0, 0, 0, 0, 0.0])
    add(axis_cam, INTR, [0.5, -0.25, 6.0], (320.5, 239.5))                                    # X - tau = (0, 0, 5) exactly
    obs += [[generic, 3, 300.0, 200.0], [2, generic, 350.0, 260.0], [nc0 - 3, 7, 310.0, 255.0]]
    return cams, intr, np.array(pts), np.array(obs, dtype=np.float64)


def update_cases():
    """(cams (n, 7), increments (n, 7)): every cell camera with a generic increment, the generic camera with every cell
    camera's [w | s] as the increment, a zero increment, the composite rotation across pi from both sides, the composite s
    through 0 (exactly, and by a sign change)"""
    cc = cell_cams()
    gen_d = np.array([0.01, -0.02, 0.015, 0.02, -0.01, 0.03, 0.05])
    gen_c = cc[24]
    cams = [c for c in cc] + [gen_c for _ in cc]
    incs = [gen_d for _ in cc] + [np.concatenate([[0.02, 0.01, -0.03], c[3:7]]) for c in cc]
    cams.append(gen_c); incs.append(np.zeros(7))
    near = _cam([0.3, -0.2, 0.5], 1, np.pi - 0.02, 0.1)                   # about e_z: increments about e_z add their angles
    for dth in (0.02 - 2e-3, 0.02 + 2e-3):
        cams.append(near); incs.append(np.concatenate([[0.01, 0.02, 0.03], dth * AXES[1], [0.01]]))
    cams.append(_cam([0.3, -0.2, 0.5], 2, 0.4, 0.3)); incs.append(np.concatenate([[0.01, 0.02, 0.03], 0.1 * AXES[0], [-0.3]]))
    cams.append(_cam([0.3, -0.2, 0.5], 2, 0.4, 1e-7)); incs.append(np.concatenate([[0.01, 0.02, 0.03], 0.1 * AXES[0], [-3e-7]]))
    return np.array(cams), np.array(incs)


# ---------------------------------------------------------------------------------------------------------------------
# scales: |error| <= C eps scale, built from the inputs (and the camera-frame depth / the composite angle of the reference)
# ---------------------------------------------------------------------------------------------------------------------
def _n(a):
    return np.linalg.norm(a, axis=-1)


def _tau_bound(v):
    """|tau| <= (|a| + |b| |w| + |c| |w|^2) |t| with a, b, c <= e^|s|"""
    w = _n(v[:, 3:6])
    return np.exp(np.abs(v[:, 6])) * (1 + w + w * w) * _n(v[:, :3])


def edge_scales(cams, intr, pts, obs, aux):
    """the projection scales of DESIGN section 18 (geometry_cases._proj_scales) with x = e^-s R^T (X - tau): the terms of x
    are bounded by e^|s| (1 + |w|)(|X| + |tau|), tau by _tau_bound; the distortion divides by 0.5 fx fy and multiplies the
    SQUARED radius, |p - c| <= (fx + fy) rho. J0: translation columns P, rotation and scale columns P times the terms of x
    (the scale column is identically zero, the reference's difference quotient of it is not)."""
    c, X, it = cams[obs[:, 0].astype(int)], pts[obs[:, 1].astype(int)], intr[obs[:, 0].astype(int)]
    es, th = np.exp(np.abs(c[:, 6])), 1 + _n(c[:, 3:6])
    sx = es * th * (_n(X) + _tau_bound(c))
    z = np.abs(aux[:, 2])
    rho = sx / z
    f = it[:, 0] + it[:, 1]
    kappa = (f * rho) ** 2 * np.abs(it[:, 4]) / (0.5 * it[:, 0] * it[:, 1])
    amp = 1 + 3 * kappa
    s_uv, s_pt = amp * f * rho * rho, amp * f / z * rho * rho
    one = np.ones((obs.shape[0], 1))
    J0 = np.concatenate([s_pt[:, None] * np.tile(one, (1, 6)), (s_pt * (1 + sx))[:, None] * np.tile(one, (1, 8))], axis=1)
    return {"J0": J0, "J1": (s_pt * es * th)[:, None] * np.tile(one, (1, 6)),
            "r": (s_uv + np.abs(obs[:, 2:4]).max(axis=1) + np.abs(it[:, 2:4]).max(axis=1))[:, None] * np.tile(one, (1, 2))}


def update_scales(cams, incs, aux):
    """t' = V^-1 (tau1 + e^s1 R1 tau2): |V^-1| <= e^|s'| up to the angle's conditioning; the rotation's logarithm loses
    1 / (pi - th') near pi (geometry_cases._near_pi) and t' is computed from it; s' = s1 + s2"""
    th = 1 + _n(cams[:, 3:6]) + _n(incs[:, 3:6])
    near = np.maximum(1.0, 1.0 / (np.pi - aux[:, 0]))
    es1, es = np.exp(np.abs(cams[:, 6])), np.exp(np.abs(cams[:, 6]) + np.abs(incs[:, 6]))
    tau = _tau_bound(cams) + es1 * th * _tau_bound(incs)
    st, sw = es * th * th * tau * near, th * near
    ss = np.maximum(np.abs(cams[:, 6]) + np.abs(incs[:, 6]), np.finfo(np.float64).tiny)
    return {"out": np.concatenate([np.tile(st[:, None], (1, 3)), np.tile(sw[:, None], (1, 3)), ss[:, None]], axis=1),
            "R": np.tile(th[:, None], (1, 9))}


# per output: 8 x the largest quotient |mirror - reference| / (eps scale) over the cases (a quotient below 1 counts as 1),
# rounded up to a power of two (DESIGN section 18's rule); tests/test_sim3_host.py recomputes the quotients and fails if a
# constant here is not that
C = {"J0": 8, "J1": 8, "r": 8, "out": 16, "R": 8}


def c_rule(q):
    return int(2 ** np.ceil(np.log2(8 * max(1.0, float(q)))))


def rodrigues(a):
    """float64 rotation matrices of axis-angle rows (n, 3) -> (n, 9) row-major, for comparing rotations as matrices"""
    a = np.asarray(a, dtype=np.float64)
    S, Cc, _, _ = formats._sim3_sinc(_n(a))
    K = formats._hat(a)
    return (np.eye(3)[None] + S[:, None, None] * K + Cc[:, None, None] * np.einsum("eij,ejk->eik", K, K)).reshape(-1, 9)


# ----------------------------------------------------------------------------------------------------------------------
# the Levenberg-Marquardt loop on the host (tests/test_sim3_host.py, tests/test_gpu_sim3_ba.py)
# ----------------------------------------------------------------------------------------------------------------------
def dense_lambda(p, alpha=0.0):
    """Lambda + alpha I and eta of a sim3_ba_linearize Problem in dense float64, every J^T Omega J term summed edge by edge"""
    dim = np.asarray(p.dim, dtype=np.int64)
    base = np.concatenate([[0], np.cumsum(dim)])
    n, no = int(base[-1]), p.v0.size
    J0, J1 = p.J0.reshape(no, 7, 2).transpose(0, 2, 1), p.J1.reshape(no, 3, 2).transpose(0, 2, 1)
    Om = p.Om.reshape(no, 2, 2)
    L, eta = np.zeros((n, n)), np.zeros(n)
    ia, ib = base[p.v0][:, None] + np.arange(7), base[p.v1][:, None] + np.arange(3)
    np.add.at(eta, ia, np.einsum("eli,elm,em->ei", J0, Om, p.r))
    np.add.at(eta, ib, np.einsum("eli,elm,em->ei", J1, Om, p.r))
    for (xa, Ja), (xb, Jb) in (((ia, J0), (ia, J0)), ((ia, J0), (ib, J1)), ((ib, J1), (ia, J0)), ((ib, J1), (ib, J1))):
        np.add.at(L, (xa[:, :, None], xb[:, None, :]), np.einsum("eli,elm,emj->eij", Ja, Om, Jb))
    L[np.diag_indices(n)] += alpha
    return L, eta


class HostSim3Path:
    """the LM path on the host: numpy linearization (the mirror), dense float64 Lambda and solve"""

    def begin(self, s):
        self.s = s
        self.trace = []     # True per accepted step, False per rejected one
        self.first_dx = None

    def linearize(self):
        self.prob = self.s.linearize()

    def max_hessian_diag(self):
        p = self.prob
        Om = p.Om.reshape(-1, 2, 2)
        return max(np.einsum("eci,eij,ecj->ec", J.reshape(-1, d, 2), Om, J.reshape(-1, d, 2)).max() for J, d in ((p.J0, 7), (p.J1, 3)))

    def chi2(self):
        self.linearize()
        return float(np.einsum("ei,eij,ej->", self.prob.r, self.prob.Om.reshape(-1, 2, 2), self.prob.r))

    def solve(self, alpha):
        L, eta = dense_lambda(self.prob, alpha)
        self.dx, self.eta = np.linalg.solve(L, eta), eta
        if self.first_dx is None:
            self.first_dx = self.dx.copy()
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
