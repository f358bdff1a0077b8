"""Deterministic float64 inputs for every kernel family of spp_geometry.hip, one case per branch cell (numpy only), the
scale of every output built from the inputs alone, and the tolerance constants c of DESIGN.md section 18.

tools/make_golden_geom_edges.py runs tests/geometry_ref.py over these and writes tests/golden/geometry_edges.npz;
tests/test_geometry_ref_host.py asserts the coverage from the branch table recorded there and measures the c below.
"""
import numpy as np

EPS = 2.0 ** -52
TWO_PI = 2 * np.pi
# one angle per cell of geometry_ref.angle_cell: 0, (0, 1e-12), (1e-12, 1e-6), within 1 % below and above 1e-6, generic,
# (pi, 2 pi), beyond 2 pi
ROT_ANGLES = [0.0, 3e-13, 5e-9, 0.995e-6, 1.005e-6, 1.3, 4.0, 7.0]


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _cat(*a):
    return np.concatenate([np.atleast_1d(np.asarray(x, dtype=np.float64)) for x in a])


def _rot(a):
    """float64 Rodrigues, for PLACING points only (no reference value depends on it)"""
    th = np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    if th < 1e-8:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K


# ---------------------------------------------------------------------------------------------------------------------
def se3_cases():
    """poses (nv, 6), edges (ne, 8) i j z: the cells of the SE(3) edge"""
    rng = np.random.default_rng(101)
    P, E = [], []

    def pose(t, r):
        P.append(_cat(t, r))
        return len(P) - 1

    def edge(i, j, zt, zr):
        E.append(_cat(i, j, zt, zr))

    # every cell of the input angle at pose 1, at pose 2 (the same pair with reversed ids) and at the measurement
    for th in ROT_ANGLES:
        ax = _unit(rng)
        i = pose(rng.normal(size=3), ax * th)
        aj = _unit(rng)
        j = pose(rng.normal(size=3), aj * 0.7)
        k = pose(rng.normal(size=3), aj * 0.84)                # 0.14 from j: the residual stays within 0.14 of the measurement
        zt, zr = rng.normal(size=3), _unit(rng) * 0.4
        edge(i, j, zt, zr)
        edge(j, i, zt, zr)
        edge(j, k, rng.normal(size=3), ax * th)
    # relative rotation about a common axis: 0, (0, 1e-4) twice, both sides of 1e-4, generic, pi - 1e-3
    for delta in (0.0, 7e-7, 3e-5, 0.99e-4, 1.01e-4, 0.8, np.pi - 1.001e-3):
        ax = _unit(rng)
        i = pose(rng.normal(size=3), ax * 0.3)
        j = pose(rng.normal(size=3), ax * (0.3 + delta))
        edge(i, j, rng.normal(size=3), _unit(rng) * 0.2)
    # w of q1^* q2 negative before canonicalisation: -2 and +2 about one axis (relative angle 4 -> 2 pi - 4)
    ax = _unit(rng)
    i, j = pose(rng.normal(size=3), ax * -2.0), pose(rng.normal(size=3), ax * 2.0)
    edge(i, j, rng.normal(size=3), _unit(rng) * 0.2)
    # residual rotation about the common axis: 0 exactly, 1, 3 (w > 0); 4 -> 2 pi - 4 and 2 pi - 3 -> 3 (w < 0)
    ax = _unit(rng)
    i, j = pose(rng.normal(size=3), ax * 0.3), pose(rng.normal(size=3), ax * 0.3)
    edge(i, j, rng.normal(size=3), np.zeros(3))
    for de, zr in ((0.5, 1.5), (-0.5, 2.5), (-1.0, 3.0), (2.5 - (TWO_PI - 3.0), 2.5)):
        ax = _unit(rng)
        i, j = pose(rng.normal(size=3), ax * 0.3), pose(rng.normal(size=3), ax * (0.3 + de))
        edge(i, j, rng.normal(size=3), ax * zr)
    # 0 < vn < 1e-12 in the expectation (poses 0 and 3e-13) and in the residual (equal rotations, measurement 3e-13)
    i, j = pose(rng.normal(size=3), np.zeros(3)), pose(rng.normal(size=3), _unit(rng) * 3e-13)
    edge(i, j, rng.normal(size=3), _unit(rng) * 0.2)
    ax = _unit(rng)
    i, j = pose(rng.normal(size=3), ax * 0.3), pose(rng.normal(size=3), ax * 0.3)
    edge(i, j, rng.normal(size=3), _unit(rng) * 3e-13)
    # translations of magnitude 1e-3, 1, 1e3
    for s in (1e-3, 1.0, 1e3):
        i, j = pose(s * rng.normal(size=3), _unit(rng) * 0.6), pose(s * rng.normal(size=3), _unit(rng) * 1.1)
        edge(i, j, s * rng.normal(size=3), _unit(rng) * 0.5)
    # gathers: an edge from a pose to itself, one id in many edges, ids in no order
    edge(5, 5, np.zeros(3), np.zeros(3))
    edge(len(P) - 1, 0, rng.normal(size=3), _unit(rng) * 0.3)
    edge(2, len(P) - 2, rng.normal(size=3), _unit(rng) * 0.3)
    return np.array(P), np.array(E)


def xyz_cases():
    """dim, flat state (poses interleaved with landmarks), obs (k, 5) pose vertex, landmark vertex, z"""
    rng = np.random.default_rng(102)
    dim, vals, obs = [], [], []

    def vertex(v):
        dim.append(len(v))
        vals.append(np.asarray(v, dtype=np.float64))
        return len(dim) - 1

    for th in ROT_ANGLES:
        p = vertex(_cat(rng.normal(size=3), _unit(rng) * th))
        l = vertex(rng.normal(size=3) * 2)
        obs.append(_cat(p, l, rng.normal(size=3)))
    for s in (1e-3, 1.0, 1e3):
        t = rng.normal(size=3)
        p = vertex(_cat(t, _unit(rng) * 0.8))
        l = vertex(t + s * rng.normal(size=3))
        obs.append(_cat(p, l, s * rng.normal(size=3)))
    # gathers: one pose sees several landmarks, one landmark is seen from several poses, ids reversed
    obs.append(_cat(10, 1, rng.normal(size=3)))
    obs.append(_cat(10, 3, rng.normal(size=3)))
    obs.append(_cat(12, 3, rng.normal(size=3)))
    obs.append(_cat(0, 21, rng.normal(size=3)))
    return np.array(dim, dtype=np.int32), np.concatenate(vals), np.array(obs)


def _ba_like(rng, stereo):
    cams, intr, pts, obs = [], [], [], []
    base = [520.0, 480.0, 320.0, 240.0]                        # fx != fy throughout
    k_gen, b_gen = (0.005, [0.12]) if stereo else (1e-3, [])

    def add(cam, k, b, X, off=(0.7, -1.3, 0.4)):
        cams.append(cam)
        intr.append(_cat(base, k, b))
        pts.append(np.asarray(X, dtype=np.float64))
        obs.append([len(cams) - 1, len(pts) - 1, off])

    for th in ROT_ANGLES:                                       # every cell of the camera's angle, the point in front
        a = _unit(rng) * th
        t = np.array([0.1, -0.2, 6.0])
        xc = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(4, 7)])
        add(_cat(t, a), k_gen, b_gen, _rot(a).T @ (xc - t))
    a, t = _unit(rng) * 0.4, np.array([0.3, 0.1, 0.5])
    add(_cat(t, a), 0.0, b_gen, _rot(a).T @ (np.array([0.6, -0.4, 5.0]) - t))               # k = 0
    # strong distortion: mono r2 k' ~ 0.3 at d = (104, 48); stereo rho k' ~ 0.3 at rho ~ 114.5
    add(_cat(np.zeros(3), _unit(rng) * 1e-3), (0.3 / 114.5 if stereo else 0.3 / 13120.0) * 500.0, b_gen, [0.8, 0.4, 4.0])
    add(np.zeros(6), k_gen, b_gen, [0.0, 0.0, 4.0])                                         # on the optical axis
    add(np.zeros(6), k_gen, b_gen, [0.3, -0.2, -3.0])                                       # behind the camera
    add(_cat([1.0, 2.0, 3.0], _unit(rng) * 2e-7), k_gen, b_gen, [100.0, -50.0, 1000.0])     # |X| ~ 1e3, small angle
    if stereo:
        add(np.zeros(6), k_gen, [0.12], [0.12, 0.0, 3.0])                                   # right rho = 0: x = b, y = 0
        add(np.zeros(6), k_gen, [0.12], [1e-12 * 3.0 / 520.0, 0.5e-12 * 3.0 / 480.0, 3.0])  # left rho ~ 1e-12
        a = _unit(rng) * 0.5
        add(_cat([0.2, 0.1, 0.3], a), k_gen, [0.0], _rot(a).T @ np.array([0.5, 0.3, 4.5]))  # b = 0
    cams, intr, pts = np.array(cams), np.array(intr), np.array(pts)
    # gathers: cameras that also see each other's points (all of these lie in front of all of them: t_z = 6, |X| < 2.6),
    # one camera and one point in several observations; the order is shuffled below
    for c in (0, 5, 6):
        for p in (5, 6, 0):
            if c != p:
                obs.append([c, p, (-0.3, 0.9, 0.2)])
    # measurement = a float64 projection + offset (any value serves: r = z - e is what is compared)
    rows = []
    for c, p, off in obs:
        x = _rot(cams[c, 3:]) @ pts[p] + cams[c, :3]
        u, v = 520.0 * x[0] / x[2] + 320.0, 480.0 * x[1] / x[2] + 240.0
        rows.append(_cat(c, p, u + off[0], v + off[1], [u + off[2]] if stereo else []))
    rows = np.array(rows)
    return cams, intr, pts, rows[rng.permutation(rows.shape[0])]


def ba_cases():
    """cams (nc, 6), intr (nc, 5), pts (np, 3), obs (no, 4) cam pt u v"""
    return _ba_like(np.random.default_rng(103), False)


def stereo_cases():
    """cams (nc, 6), intr (nc, 6), pts (np, 3), obs (no, 5) cam pt u v u_right"""
    return _ba_like(np.random.default_rng(104), True)


def se2_cases():
    """poses (nv, 3), edges (ne, 5) i j z"""
    rng = np.random.default_rng(105)
    ang = [0.4, -2.9, 50.3, -17.9, 6.9, -7.1, 1.1, 3.0]
    poses = np.array([_cat(rng.normal(size=2) * 3, a) for a in ang])
    E = []

    def edge(i, j, dz):
        ha = np.fmod(poses[j, 2] - poses[i, 2], TWO_PI)
        E.append(_cat(i, j, rng.normal(size=2), ha + dz))

    for i, j in ((0, 1), (1, 0), (2, 3), (3, 2), (4, 5), (5, 4), (0, 2), (3, 6), (7, 1)):    # angles outside, negative
        edge(i, j, 0.05)
    for dz in (0.5, 4.0, -4.0, 7.0, -7.0):                  # the three arms of the error clamp, with and without a wrap
        edge(6, 7, dz)
    for dz in (np.pi - 5e-7, np.pi + 5e-7, -np.pi + 5e-7, -np.pi - 5e-7):    # within 1e-6 of +-pi, from both sides
        edge(0, 6, dz)
    edge(4, 4, 0.0)                                          # an edge from a pose to itself
    return poses, np.array(E)


def rb_cases():
    """dim, flat state (3-wide poses interleaved with 2-wide landmarks), obs (k, 4) pose vertex, landmark vertex, range, bearing"""
    rng = np.random.default_rng(106)
    dim, vals, obs = [], [], []

    def vertex(v):
        dim.append(len(v))
        vals.append(np.asarray(v, dtype=np.float64))
        return len(dim) - 1

    def case(p, d, beta, dz):
        pv = vertex(p)
        lv = vertex([p[0] + d * np.cos(beta), p[1] + d * np.sin(beta)])
        obs.append(_cat(pv, lv, d + 0.01, np.fmod(beta - p[2], TWO_PI) + dz))

    case([0.5, -0.25, 0.3], 0.0, 0.0, 0.1)                   # d = 0 exactly
    case([0.5, -0.25, 0.3], 5e-6, 0.7, 0.1)                  # below the floor
    case([0.5, -0.25, -0.4], 2e-5, 2.1, -0.1)                # just above it
    case([1.5, 2.0, 0.9], 3.7, -1.2, 0.2)                    # generic
    case([1.5, 2.0, 0.2], 2.0, np.pi - 1e-9, 0.05)           # bearing across the atan2 cut: just below +pi
    case([1.5, 2.0, 0.2], 2.0, -np.pi + 1e-9, 0.05)          # ... just above -pi
    case([-3.0, 1.0, 40.7], 1.3, 0.4, 0.0)                   # pose angle outside [-2 pi, 2 pi]
    case([-3.0, 1.0, -9.9], 1.3, 2.4, 0.0)
    for dz in (4.0, -4.0, np.pi - 5e-7, -np.pi + 5e-7):      # the arms of the bearing error, near +-pi
        case([0.2, 0.1, 0.5], 1.0, 0.8, dz)
    obs.append(_cat(6, 9, 1.0, 0.3))                         # gathers: a pose with another pose's landmark, reversed order
    obs.append(_cat(12, 3, 2.0, -0.3))
    return np.array(dim, dtype=np.int32), np.concatenate(vals), np.array(obs)


def plus_cases():
    """p (n, 6), d (n, 6): the cells of x (+) dx on SE(3)"""
    rng = np.random.default_rng(107)
    P, D = [], []

    def case(p, d):
        P.append(_cat(p))
        D.append(_cat(d))

    for th in ROT_ANGLES:                                    # every cell of the pose's angle and of the increment's
        case(_cat(rng.normal(size=3), _unit(rng) * th), _cat(rng.normal(size=3) * 0.1, _unit(rng) * 0.05))
        case(_cat(rng.normal(size=3), _unit(rng) * 0.8), _cat(rng.normal(size=3) * 0.1, _unit(rng) * th))
    case(_cat(rng.normal(size=3), _unit(rng) * 0.8), np.zeros(6))          # zero increment
    case(_cat(rng.normal(size=3), _unit(rng) * 4.0), np.zeros(6))          # ... on a pose beyond pi
    case(_cat(rng.normal(size=3), np.zeros(3)), _cat(0.1, 0.2, 0.3, np.zeros(3)))   # composite with vn = 0
    ax = _unit(rng)
    case(_cat(rng.normal(size=3), ax * 3.0), _cat(rng.normal(size=3) * 0.1, ax * 0.3))    # crosses pi: the w < 0 flip
    case(_cat(rng.normal(size=3), ax * 3.0), _cat(rng.normal(size=3) * 0.1, ax * 0.1))    # stops short of pi
    case(_cat(rng.normal(size=3), ax * -3.0), _cat(rng.normal(size=3) * 0.1, ax * -0.4))
    case(_cat(rng.normal(size=3), np.zeros(3)), _cat(rng.normal(size=3) * 0.1, _unit(rng) * 3e-13))   # 0 < vn < 1e-12
    case(_cat(rng.normal(size=3), np.zeros(3)), _cat(rng.normal(size=3) * 0.1, _unit(rng) * 5e-9))    # vn just above
    for s in (1e-3, 1.0, 1e3):
        case(_cat(s * rng.normal(size=3), _unit(rng) * 1.2), _cat(s * 0.1 * rng.normal(size=3), _unit(rng) * 0.02))
    return np.array(P), np.array(D)


def upd2_cases():
    """p (n, 3), d (n, 3): 2D pose (+), sums inside and outside [-2 pi, 2 pi]"""
    p = np.array([[0.5, 1.0, 0.4], [1.0, -2.0, 6.2], [0.0, 3.0, -6.2], [7.0, 1.0, 50.3], [2.0, 2.0, 3.0], [1.0, 1.0, -2.0]])
    d = np.array([[0.1, -0.1, 0.1], [0.2, 0.3, 0.2], [0.1, 0.1, -0.2], [-0.5, 0.5, 1.0], [0.0, 0.0, -3.0], [0.3, 0.2, 0.5]])
    return p, d


def inputs():
    """every family's inputs as one dict of arrays (the input half of tests/golden/geometry_edges.npz)"""
    g = {}
    g["se3_poses"], g["se3_edges"] = se3_cases()
    g["xyz_dim"], g["xyz_state"], g["xyz_obs"] = xyz_cases()
    g["ba_cams"], g["ba_intr"], g["ba_pts"], g["ba_obs"] = ba_cases()
    g["stereo_cams"], g["stereo_intr"], g["stereo_pts"], g["stereo_obs"] = stereo_cases()
    g["se2_poses"], g["se2_edges"] = se2_cases()
    g["rb_dim"], g["rb_state"], g["rb_obs"] = rb_cases()
    g["plus_p"], g["plus_d"] = plus_cases()
    g["upd2_p"], g["upd2_d"] = upd2_cases()
    return g


def offsets(dim):
    base = np.zeros(len(dim) + 1, dtype=np.int64)
    np.cumsum(dim, out=base[1:])
    return base


# ---------------------------------------------------------------------------------------------------------------------
# scales: |error| <= c eps scale. Built from the INPUTS (and from angles the reference derived from the inputs: th_e, th_r,
# the camera-frame depth), never from an output under test.
# ---------------------------------------------------------------------------------------------------------------------
def _n(a):
    return np.linalg.norm(a, axis=-1)


def _near_pi(th):
    """log(R) loses 1 / (pi - th) near pi (R -> axis-angle through a matrix, as the float64 mirrors do it)"""
    return np.maximum(1.0, 1.0 / (np.pi - th))


def se3_scales(g):
    P, E = g["se3_poses"], g["se3_edges"]
    p1, p2, z = P[E[:, 0].astype(int)], P[E[:, 1].astype(int)], E[:, 2:8]
    ne = E.shape[0]
    th = 1 + _n(p1[:, 3:]) + _n(p2[:, 3:])
    dt = _n(p2[:, :3] - p1[:, :3])
    st = th * (1 + dt)                                       # entries of e_t, [e_t]x, R_e
    sr = th * _near_pi(g["se3_aux"][:, 0])                   # entries of Jr^-1, Jr^-1 R_e^T
    rows = np.concatenate([np.tile(st[:, None], (1, 3)), np.tile(sr[:, None], (1, 3))], axis=1)    # (ne, 6) by row
    J = np.tile(rows[:, None, :], (1, 6, 1)).reshape(ne, 36)                                        # column-major
    r = np.concatenate([np.tile((th * (dt + _n(z[:, :3]) + 1))[:, None], (1, 3)),
                        np.tile(((th + _n(z[:, 3:])) * _near_pi(g["se3_aux"][:, 1]))[:, None], (1, 3))], axis=1)
    return {"J0": J, "J1": J, "r": r}


def xyz_scales(g):
    x, base, obs = g["xyz_state"], offsets(g["xyz_dim"]), g["xyz_obs"]
    p = x[base[obs[:, 0].astype(int)][:, None] + np.arange(6)]
    l = x[base[obs[:, 1].astype(int)][:, None] + np.arange(3)]
    th = 1 + _n(p[:, 3:])
    d = _n(l - p[:, :3])
    k = obs.shape[0]
    return {"J0": np.tile((th * (1 + d))[:, None], (1, 18)), "J1": np.tile(th[:, None], (1, 9)),
            "r": np.tile((th * d + _n(obs[:, 2:5]))[:, None], (1, 3))}


def _proj_scales(g, fam, stereo):
    cams, intr, pts, obs = (g[fam + k] for k in ("_cams", "_intr", "_pts", "_obs"))
    c, X = cams[obs[:, 0].astype(int)], pts[obs[:, 1].astype(int)]
    it = intr[obs[:, 0].astype(int)]
    th = 1 + _n(c[:, 3:])
    sx = th * _n(X) + _n(c[:, :3]) + (np.abs(it[:, 5]) if stereo else 0.0)    # |terms| of x = R X + t (- b e0)
    z = np.abs(g[fam + "_aux"][:, 2])                                           # camera-frame depth, from the reference
    rho = sx / z                                                                # >= 1: conditioning of x / z
    f = it[:, 0] + it[:, 1]
    kp = np.abs(it[:, 4]) / (0.5 * f)
    kappa = (f * rho) ** (1 if stereo else 2) * kp                              # bound of the distortion term of g
    amp = 1 + 3 * kappa
    s_uv = amp * f * rho * rho
    s_pt = amp * f / z * rho * rho
    nr, w = (3, 9) if stereo else (2, 6)
    J0 = np.concatenate([np.tile(s_pt[:, None], (1, w)), np.tile((s_pt * (1 + _n(X)))[:, None], (1, w))], axis=1)
    return {"J0": J0, "J1": np.tile(s_pt[:, None], (1, w)),
            "r": np.tile((s_uv + np.abs(obs[:, 2:]).max(axis=1) + np.abs(it[:, 2:4]).max(axis=1))[:, None], (1, nr))}


def ba_scales(g):
    return _proj_scales(g, "ba", False)


def stereo_scales(g):
    return _proj_scales(g, "stereo", True)


def se2_scales(g):
    P, E = g["se2_poses"], g["se2_edges"]
    p1, p2 = P[E[:, 0].astype(int)], P[E[:, 1].astype(int)]
    ne = E.shape[0]
    d = _n(p2[:, :2] - p1[:, :2])
    sa = 1 + np.abs(p1[:, 2]) + np.abs(p2[:, 2]) + np.abs(E[:, 4])
    J = np.tile((1 + d)[:, None], (1, 9))
    return {"J0": J, "J1": J, "r": np.stack([d + np.abs(E[:, 2]), d + np.abs(E[:, 3]), sa], axis=1)}


def rb_scales(g):
    x, base, obs = g["rb_state"], offsets(g["rb_dim"]), g["rb_obs"]
    p = x[base[obs[:, 0].astype(int)][:, None] + np.arange(3)]
    l = x[base[obs[:, 1].astype(int)][:, None] + np.arange(2)]
    d = np.maximum(g["rb_aux"][:, 0], 1e-5)                  # the floored range, from the reference
    sa = 1 + np.pi + np.abs(p[:, 2]) + np.abs(obs[:, 3])
    one, inv = np.ones_like(d), 1.0 / d                      # row 0 entries are cosines, row 1 entries are cosines / d
    return {"J0": np.stack([one, inv, one, inv, one, one], axis=1), "J1": np.stack([one, inv, one, inv], axis=1),
            "r": np.stack([d + np.abs(obs[:, 2]), sa], axis=1)}


def plus_scales(g):
    p, d = g["plus_p"], g["plus_d"]
    th = 1 + _n(p[:, 3:]) + _n(d[:, 3:])
    st = _n(p[:, :3]) + th * _n(d[:, :3])
    return {"out": np.concatenate([np.tile(st[:, None], (1, 3)), np.tile((th * _near_pi(g["plus_aux"][:, 0]))[:, None], (1, 3))],
                                  axis=1), "R": np.tile(th[:, None], (1, 9))}


def upd2_scales(g):
    p, d = g["upd2_p"], g["upd2_d"]
    return {"out": np.abs(p) + np.abs(d) + np.array([0, 0, 1.0])}


SCALES = {"se3": se3_scales, "xyz": xyz_scales, "ba": ba_scales, "stereo": stereo_scales, "se2": se2_scales, "rb": rb_scales,
          "plus": plus_scales, "upd2": upd2_scales}

# c per family and output: 8 x the largest quotient |mirror - reference| / (eps scale) measured on the fixture (a quotient
# below 1 counts as 1: one rounding of a number of the scale's size), rounded up to a power of two; never above 4096.
# tests/test_geometry_ref_host.py recomputes the quotients and fails if a constant here is not that.
C = {"se3": {"J0": 16, "J1": 8, "r": 8}, "xyz": {"J0": 8, "J1": 8, "r": 8}, "ba": {"J0": 8, "J1": 8, "r": 8},
     "stereo": {"J0": 8, "J1": 8, "r": 8}, "se2": {"J0": 8, "J1": 8, "r": 8}, "rb": {"J0": 8, "J1": 8, "r": 8},
     "plus": {"out": 8, "R": 8}, "upd2": {"out": 8}}


def c_rule(q):
    """the constant the largest mirror quotient q asks for"""
    return int(2 ** np.ceil(np.log2(8 * max(1.0, float(q)))))


def rodrigues(a):
    """float64 rotation matrices of axis-angle rows (n, 3) -> (n, 9) row-major, for comparing rotations as matrices"""
    a = np.asarray(a, dtype=np.float64)
    out = np.empty((a.shape[0], 9))
    for i, v in enumerate(a):
        th = np.linalg.norm(v)
        K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
        A, B = (1 - th * th / 6, 0.5 - th * th / 24) if th < 1e-6 else (np.sin(th) / th, 2 * np.sin(th / 2) ** 2 / th ** 2)
        out[i] = (np.eye(3) + A * K + B * K @ K).ravel()
    return out
