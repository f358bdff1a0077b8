"""Seeded synthetic problems shaped like the five BASELINE.json configs. numpy only.

The real datasets (manhattanOlson3500, sphere2500, BAL Ladybug-49, Venice-871) are not available
offline, so every config is a *shape-matched synthetic*: same vertex/edge counts, same block
widths, plausible geometry. A problem is the INPUT of the hot path: one homogeneous group of binary
edges with per-edge Jacobians J0 (rd x d0), J1 (rd x d1), information Omega (rd x rd) and residual r
-- i.e. the outputs of the reference's Calculate_Jacobians_Expectation_Error
(include/slam/BaseTypes_Binary.h:763-765), which stays reference code.
All per-edge arrays are column-major blocks flattened edge by edge.
"""
import numpy as np


class Problem(dict):
    """dict with attribute access: dim, v0, v1, d0, d1, rd, J0, J1, Om, r, unary_vertex, damping, name.
    unary_vertex: the vertex whose diagonal block receives the unit unary factor -- vertex 0 in the reference's
    default build (__AUTO_UNARY_FACTOR_ON_VERTEX_ZERO, include/slam/FlatSystem.h:331-337; pinned by
    tests/golden/ba_lambda.npz, where vertex 0 is a landmark), whatever its type."""
    __getattr__ = dict.__getitem__


# ------------------------------------------------------------------------------------------------
# bundle adjustment (configs 3, 4, 5): cameras (6) + points (3), 2-d reprojection residuals
# ------------------------------------------------------------------------------------------------
def _track_lengths(rng, npts, nobs, kmin, kmax, heavy_tail):
    mean = nobs / float(npts)
    if heavy_tail:
        k = kmin + rng.geometric(1.0 / (mean - kmin + 1.0), size=npts) - 1
    else:
        lo = int(np.floor(mean))
        k = np.full(npts, lo, dtype=np.int64)
        k[rng.permutation(npts)[:nobs - lo * npts]] += 1
    k = np.clip(k, kmin, kmax).astype(np.int64)
    diff = int(nobs - k.sum())
    while diff != 0:  # nudge random tracks until the observation count is exact
        step = 1 if diff > 0 else -1
        ok = np.flatnonzero((k + step >= kmin) & (k + step <= kmax))
        pick = rng.choice(ok, size=min(abs(diff), ok.size), replace=False)
        k[pick] += step
        diff = int(nobs - k.sum())
    return k


def ba_problem(nc, npts, nobs, seed, heavy_tail=True, interleave=False, spread=0.12, name="ba"):
    """nc cameras on a circle looking at the origin, npts points in a cube, exactly nobs observations.
    Point j is seen by k_j distinct cameras drawn around a centre camera (window ~ spread * nc), which
    yields a banded-to-dense reduced camera system. interleave=True shuffles vertex ids so that about
    half of the camera-point blocks have (point id < camera id) and are stored transposed
    (reference BaseTypes_Binary.h:783-806)."""
    rng = np.random.default_rng(seed)
    kmax = min(nc, 64)
    k = _track_lengths(rng, npts, nobs, 2, kmax, heavy_tail)
    centre = rng.integers(0, nc, size=npts)
    cam_of = np.empty(nobs, dtype=np.int64)
    pt_of = np.repeat(np.arange(npts, dtype=np.int64), k)
    start = np.zeros(npts + 1, dtype=np.int64)
    np.cumsum(k, out=start[1:])
    half = max(2, int(spread * nc))
    for kk in np.unique(k):
        idx = np.flatnonzero(k == kk)
        win = min(nc, max(2 * half + 1, int(kk)))
        # kk distinct offsets in a window: argsort of random keys
        offs = np.argsort(rng.random((idx.size, win)), axis=1)[:, :kk] - win // 2
        cams = np.sort((centre[idx, None] + offs) % nc, axis=1)
        pos = start[idx, None] + np.arange(kk)[None, :]
        cam_of[pos.ravel()] = cams.ravel()
    # geometry
    th = 2 * np.pi * np.arange(nc) / nc
    C = np.stack([10 * np.cos(th), 10 * np.sin(th), 0.5 * np.sin(3 * th)], axis=1)
    z = -C / np.linalg.norm(C, axis=1, keepdims=True)
    up = np.array([0.0, 0.0, 1.0])
    x = np.cross(up[None, :], z)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    y = np.cross(z, x)
    R = np.stack([x, y, z], axis=1)  # rows = camera axes (world -> camera)
    X = rng.uniform(-2, 2, size=(npts, 3))
    pc = np.einsum("eij,ej->ei", R[cam_of], X[pt_of] - C[cam_of])
    f = 500.0
    iz = 1.0 / pc[:, 2]
    Kp = np.zeros((nobs, 2, 3))
    Kp[:, 0, 0] = f * iz
    Kp[:, 1, 1] = f * iz
    Kp[:, 0, 2] = -f * pc[:, 0] * iz * iz
    Kp[:, 1, 2] = -f * pc[:, 1] * iz * iz
    Jp = np.einsum("eij,ejk->eik", Kp, R[cam_of])            # d(u,v)/dX
    skew = np.zeros((nobs, 3, 3))
    skew[:, 0, 1], skew[:, 0, 2] = -pc[:, 2], pc[:, 1]
    skew[:, 1, 0], skew[:, 1, 2] = pc[:, 2], -pc[:, 0]
    skew[:, 2, 0], skew[:, 2, 1] = -pc[:, 1], pc[:, 0]
    Jc = np.concatenate([Kp, -np.einsum("eij,ejk->eik", Kp, skew)], axis=2)  # d(u,v)/d(t, w)
    r = rng.normal(0, 0.5, size=(nobs, 2)) + 0.02 * f * iz[:, None] * rng.normal(0, 1, size=(nobs, 2))
    Om = np.tile(np.eye(2).ravel(), (nobs, 1))
    # vertex ids
    nv = nc + npts
    if interleave:
        perm = rng.permutation(nv)
        cam_id, pt_id = perm[:nc], perm[nc:]
    else:
        cam_id, pt_id = np.arange(nc), nc + np.arange(npts)
    dim = np.empty(nv, dtype=np.int32)
    dim[cam_id] = 6
    dim[pt_id] = 3
    # Levenberg-Marquardt damping as the reference applies it on BA inputs (slam_app switches to LM,
    # src/slam_app/Main.cpp:203-208): alpha0 = 1e-3 * largest diagonal entry of any vertex Hessian
    # (NonlinearSolver_Lambda_LM.h:151-199)
    h0 = np.einsum("eri,eri->ei", Jc, Jc).max()
    h1 = np.einsum("eri,eri->ei", Jp, Jp).max()
    return Problem(name=name, dim=dim, v0=cam_id[cam_of], v1=pt_id[pt_of], d0=6, d1=3, rd=2,
                   J0=np.ascontiguousarray(Jc.transpose(0, 2, 1)).reshape(nobs, 12),  # col-major 2x6
                   J1=np.ascontiguousarray(Jp.transpose(0, 2, 1)).reshape(nobs, 6),   # col-major 2x3
                   Om=Om, r=r, unary_vertex=0, damping=1e-3 * float(max(h0, h1)),
                   nc=nc, npts=npts, geometry=dict(R=R, C=C, X=X, f=f, cam_of=cam_of, pt_of=pt_of, cam_id=cam_id, pt_id=pt_id))


def ba_states(prob):
    """The same scene in the REFERENCE's parameterization, as input of spp_ba_linearize_device: cameras
    [t | axis-angle] (world -> camera, CVertexCam), intrinsics fx fy cx cy k, points, and measurements
    z = projection + the problem's residual (so that the device residual reproduces prob.r).
    Returns dict(cams (nc,6), intr (nc,5), points (np,3), meas (no,2), cam_of, pt_of int32,
    cam_dxoff, pt_dxoff int64: scalar offset of every vertex in the solution vector)."""
    from scipy.spatial.transform import Rotation
    g = prob.geometry
    R, C, X, f = g["R"], g["C"], g["X"], g["f"]
    nc, npts = R.shape[0], X.shape[0]
    cams = np.concatenate([-np.einsum("cij,cj->ci", R, C), Rotation.from_matrix(R).as_rotvec()], axis=1)
    intr = np.tile(np.array([f, f, 0.0, 0.0, 0.0]), (nc, 1))
    pc = np.einsum("eij,ej->ei", R[g["cam_of"]], X[g["pt_of"]] - C[g["cam_of"]])
    uv = f * pc[:, :2] / pc[:, 2:3]
    base = np.zeros(prob.dim.size + 1, dtype=np.int64)
    np.cumsum(prob.dim, out=base[1:])
    return dict(cams=cams, intr=intr, points=X.copy(), meas=uv + prob.r, cam_of=g["cam_of"].astype(np.int32),
                pt_of=g["pt_of"].astype(np.int32), cam_dxoff=base[g["cam_id"]].copy(), pt_dxoff=base[g["pt_id"]].copy())


# ------------------------------------------------------------------------------------------------
# 2D pose graph (config 1): manhattan-world random walk, 3x3 blocks
# ------------------------------------------------------------------------------------------------
def se2_problem(n=3500, n_loops=2099, seed=1234, name="manhattan3500"):
    rng = np.random.default_rng(seed)
    heading = np.zeros(n, dtype=np.int64)
    turn = rng.random(n) < 0.25
    heading[1:] = np.cumsum(np.where(turn[1:], rng.choice([-1, 1], size=n - 1), 0)) % 4
    step = np.stack([np.cos(heading * np.pi / 2), np.sin(heading * np.pi / 2)], axis=1).round()
    t = np.zeros((n, 2))
    t[1:] = np.cumsum(step[:-1], axis=0)
    theta = heading * np.pi / 2
    i0 = np.arange(n - 1)
    i1 = i0 + 1
    # loop closures between non-consecutive poses closer than 1.5
    from scipy.spatial import cKDTree
    pairs = cKDTree(t).query_pairs(1.5, output_type="ndarray")
    pairs = pairs[np.abs(pairs[:, 0] - pairs[:, 1]) > 1]
    pick = rng.permutation(pairs.shape[0])[:n_loops]
    lc = pairs[np.sort(pick)]
    flip = rng.random(lc.shape[0]) < 0.5  # some closures point backwards: exercises the reversed-id path
    a = np.where(flip, lc[:, 1], lc[:, 0])
    b = np.where(flip, lc[:, 0], lc[:, 1])
    v0 = np.concatenate([i0, a])
    v1 = np.concatenate([i1, b])
    ne = v0.size
    # estimate = ground truth + noise (linearization point)
    te = t + rng.normal(0, 0.05, size=t.shape)
    the = theta + rng.normal(0, 0.02, size=n)
    c, s = np.cos(the[v0]), np.sin(the[v0])
    d = te[v1] - te[v0]
    J0 = np.zeros((ne, 3, 3))
    J1 = np.zeros((ne, 3, 3))
    J0[:, 0, 0], J0[:, 0, 1], J0[:, 0, 2] = -c, -s, -s * d[:, 0] + c * d[:, 1]
    J0[:, 1, 0], J0[:, 1, 1], J0[:, 1, 2] = s, -c, -c * d[:, 0] - s * d[:, 1]
    J0[:, 2, 2] = -1
    J1[:, 0, 0], J1[:, 0, 1] = c, s
    J1[:, 1, 0], J1[:, 1, 1] = -s, c
    J1[:, 2, 2] = 1
    # residual = measurement (truth + sensor noise) - prediction at the estimate
    ct, st = np.cos(theta[v0]), np.sin(theta[v0])
    dt = t[v1] - t[v0]
    zmeas = np.stack([ct * dt[:, 0] + st * dt[:, 1], -st * dt[:, 0] + ct * dt[:, 1], theta[v1] - theta[v0]], axis=1)
    zmeas += rng.normal(0, 1, size=zmeas.shape) * np.array([0.03, 0.03, 0.01])
    pred = np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1], the[v1] - the[v0]], axis=1)
    r = zmeas - pred
    r[:, 2] = (r[:, 2] + np.pi) % (2 * np.pi) - np.pi
    Om = np.tile(np.diag([1111.11, 1111.11, 10000.0]).ravel(), (ne, 1))
    return Problem(name=name, dim=np.full(n, 3, dtype=np.int32), v0=v0, v1=v1, d0=3, d1=3, rd=3,
                   J0=np.ascontiguousarray(J0.transpose(0, 2, 1)).reshape(ne, 9),
                   J1=np.ascontiguousarray(J1.transpose(0, 2, 1)).reshape(ne, 9),
                   Om=Om, r=r, unary_vertex=0, damping=0.0,
                   geometry=dict(kind="se2", poses=np.concatenate([te, the[:, None]], axis=1), meas=zmeas))


# ------------------------------------------------------------------------------------------------
# 3D pose graph (config 2): sphere, 6x6 blocks
# ------------------------------------------------------------------------------------------------
def _rot_z(a):
    c, s = np.cos(a), np.sin(a)
    R = np.zeros(a.shape + (3, 3))
    R[..., 0, 0], R[..., 0, 1], R[..., 1, 0], R[..., 1, 1], R[..., 2, 2] = c, -s, s, c, 1
    return R


def _rot_y(a):
    c, s = np.cos(a), np.sin(a)
    R = np.zeros(a.shape + (3, 3))
    R[..., 0, 0], R[..., 0, 2], R[..., 2, 0], R[..., 2, 2], R[..., 1, 1] = c, s, -s, c, 1
    return R


def _skew(v):
    S = np.zeros(v.shape[:-1] + (3, 3))
    S[..., 0, 1], S[..., 0, 2] = -v[..., 2], v[..., 1]
    S[..., 1, 0], S[..., 1, 2] = v[..., 2], -v[..., 0]
    S[..., 2, 0], S[..., 2, 1] = -v[..., 1], v[..., 0]
    return S


def se3_problem(rings=50, per_ring=50, seed=2500, name="sphere2500"):
    rng = np.random.default_rng(seed)
    n = rings * per_ring
    ring = np.repeat(np.arange(rings), per_ring)
    k = np.tile(np.arange(per_ring), rings)
    az = 2 * np.pi * k / per_ring
    el = np.pi * (ring + 1) / (rings + 1) - np.pi / 2
    t = 50 * np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], axis=1)
    R = _rot_z(az) @ _rot_y(-el)
    i0 = np.arange(n - 1)
    i1 = i0 + 1                               # 2499 odometry edges along the spiral
    r0 = np.arange(n - per_ring)
    r1 = r0 + per_ring                        # 2450 ring-to-ring edges
    v0 = np.concatenate([i0, r0])
    v1 = np.concatenate([i1, r1])
    ne = v0.size
    te = t + rng.normal(0, 0.3, size=t.shape)
    Re = R @ (np.eye(3) + _skew(rng.normal(0, 0.02, size=(n, 3))))
    Rt = Re[v0].transpose(0, 2, 1)
    d = np.einsum("eij,ej->ei", Rt, te[v1] - te[v0])
    Rij = Rt @ Re[v1]
    J0 = np.zeros((ne, 6, 6))
    J1 = np.zeros((ne, 6, 6))
    J0[:, :3, :3] = -Rt
    J0[:, :3, 3:] = _skew(d)
    J0[:, 3:, 3:] = -Rij.transpose(0, 2, 1)
    J1[:, :3, :3] = Rt
    J1[:, 3:, 3:] = np.eye(3)
    r = rng.normal(0, 1, size=(ne, 6)) * np.array([0.05, 0.05, 0.05, 0.01, 0.01, 0.01]) + \
        0.1 * rng.normal(0, 1, size=(ne, 6)) * np.array([1, 1, 1, 0.05, 0.05, 0.05])
    Om = np.tile(np.diag([400.0] * 3 + [1e4] * 3).ravel(), (ne, 1))
    return Problem(name=name, dim=np.full(n, 6, dtype=np.int32), v0=v0, v1=v1, d0=6, d1=6, rd=6,
                   J0=np.ascontiguousarray(J0.transpose(0, 2, 1)).reshape(ne, 36),
                   J1=np.ascontiguousarray(J1.transpose(0, 2, 1)).reshape(ne, 36),
                   Om=Om, r=r, unary_vertex=0, damping=0.0, geometry=dict(kind="se3", t=t, R=R, te=te, Re=Re, seed=seed))


def landmark2d_problem(n_poses=80, n_lm=200, seed=32, interleave=False, name="lm2d_small"):
    """2D poses (3) observing 2D point landmarks (2): ONE edge group (3, 2, 2) -- the pose-landmark edges of
    victoria-park-style SLAM (CEdgePoseLandmark2D, include/slam/SE2_Types.h; range-bearing Jacobians of
    C2DJacobians::Observation2D_RangeBearing, 2DSolverBase.h:420+). Every pose sees some landmarks and every
    landmark is seen at least twice, so Lambda is positive definite with the unary factor on the first pose."""
    rng = np.random.default_rng(seed)
    nv = n_poses + n_lm
    ids = rng.permutation(nv) if interleave else np.arange(nv)
    pose_id, lm_id = ids[:n_poses], ids[n_poses:]
    P = np.concatenate([rng.uniform(0, 30, size=(n_poses, 2)), rng.uniform(-np.pi, np.pi, size=(n_poses, 1))], axis=1)
    Lm = rng.uniform(0, 30, size=(n_lm, 2))
    from scipy.spatial import cKDTree
    _, near = cKDTree(P[:, :2]).query(Lm, k=4)                    # each landmark: its 4 nearest poses
    po = near.ravel()
    lo = np.repeat(np.arange(n_lm), 4)
    seen = np.zeros(n_poses, dtype=bool)
    seen[po] = True
    extra = np.flatnonzero(~seen)                                 # poses that saw nothing: give them their nearest landmark
    if extra.size:
        _, nl = cKDTree(Lm).query(P[extra, :2], k=2)
        po = np.concatenate([po, np.repeat(extra, 2)])
        lo = np.concatenate([lo, nl.ravel()])
    ne = po.size
    d = Lm[lo] - P[po, :2]
    q = (d ** 2).sum(axis=1)
    sq = np.sqrt(q)
    J0 = np.zeros((ne, 2, 3))                                     # d(range, bearing) / d(x, y, theta)
    J1 = np.zeros((ne, 2, 2))                                     # d(range, bearing) / d(lx, ly)
    J0[:, 0, 0], J0[:, 0, 1] = -d[:, 0] / sq, -d[:, 1] / sq
    J0[:, 1, 0], J0[:, 1, 1], J0[:, 1, 2] = d[:, 1] / q, -d[:, 0] / q, -1
    J1[:, 0, 0], J1[:, 0, 1] = d[:, 0] / sq, d[:, 1] / sq
    J1[:, 1, 0], J1[:, 1, 1] = -d[:, 1] / q, d[:, 0] / q
    dim = np.empty(nv, dtype=np.int32)
    dim[pose_id], dim[lm_id] = 3, 2
    Om = np.tile(np.diag([100.0, 2500.0]).ravel(), (ne, 1))
    r = rng.normal(0, 1, size=(ne, 2)) * np.array([0.1, 0.02])
    return Problem(name=name, dim=dim, v0=pose_id[po], v1=lm_id[lo], d0=3, d1=2, rd=2,
                   J0=np.ascontiguousarray(J0.transpose(0, 2, 1)).reshape(ne, 6),
                   J1=np.ascontiguousarray(J1.transpose(0, 2, 1)).reshape(ne, 4),
                   Om=Om, r=r, unary_vertex=0, damping=1e-2)


def slam2d_problem(n_poses=60, n_lm=90, seed=68, interleave=False, name="slam2d", views=(2, 5), window=6):
    """2D landmark SLAM as a real dataset has it (victoria-park style): a planar trajectory with noisy odometry
    (CEdgePose2D) and n_poses // 5 loop closures, landmarks each seen from 2..5 nearby poses by noisy range-bearing
    (CEdgePoseLandmark2D) -- two edge groups, (3, 3, 3) and (3, 2, 2), over the same vertices. Geometrically consistent:
    the measurements come from a ground truth, the initial estimate is dead reckoning along the odometry, every landmark
    starts where its first observation puts it. interleave=True shuffles the vertex ids (vertex 0 stays the first pose,
    which carries the unary factor), so that landmarks sit between the poses and about half of the pose-landmark
    blocks are stored transposed. The edges are in the order of an incremental run: each when its later pose arrives.
    views / window: every landmark is seen from views[0] .. views[1] poses at most `window` steps from its centre pose
    (victoria-park has few landmarks seen many times: 6969 poses, 151 landmarks, about 3600 observations).
    Returns Problem(dim, state (flat, laid out by dim), odo (m, 5), odo_info, odo_seq, obs (k, 4) pose landmark range
    bearing, obs_info, obs_seq, pose_id, lm_id, truth, unary_vertex)."""
    rng = np.random.default_rng(seed)
    nv = n_poses + n_lm
    if interleave:
        ids = 1 + rng.permutation(nv - 1)
        pose_id, lm_id = np.concatenate([[0], ids[:n_poses - 1]]), ids[n_poses - 1:]
    else:
        pose_id, lm_id = np.arange(n_poses), n_poses + np.arange(n_lm)
    # ground truth: unit steps, slowly turning
    th = np.cumsum(np.concatenate([[0.0], rng.normal(0.05, 0.25, size=n_poses - 1)]))
    xy = np.zeros((n_poses, 2))
    xy[1:] = np.cumsum(np.stack([np.cos(th[:-1]), np.sin(th[:-1])], axis=1), axis=0)
    P = np.concatenate([xy, th[:, None]], axis=1)

    def rel(i, j):  # pose j in the frame of pose i
        c, s = np.cos(P[i, 2]), np.sin(P[i, 2])
        d = P[j, :2] - P[i, :2]
        return np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1], P[j, 2] - P[i, 2]], axis=1)

    oi = np.arange(n_poses - 1)
    oj = oi + 1
    lc = np.sort(np.stack([rng.choice(n_poses, size=2, replace=False) for _ in range(n_poses // 5)]), axis=1)
    oi, oj = np.concatenate([oi, lc[:, 0]]), np.concatenate([oj, lc[:, 1]])
    # wheel odometry along the chain, loop closures from a four times finer sensor (scan matching): the dead-reckoned
    # estimate then misses the closures by tens of their sigmas while staying inside Gauss-Newton's basin
    sig = np.where((np.arange(oi.size) < n_poses - 1)[:, None], np.array([0.02, 0.02, 0.004]), np.array([0.005, 0.005, 0.001]))
    z_odo = rel(oi, oj) + rng.normal(0, 1, size=(oi.size, 3)) * sig
    odo_info = np.zeros((oi.size, 3, 3))
    odo_info[:, [0, 1, 2], [0, 1, 2]] = 1.0 / sig ** 2
    # landmarks: 3 .. 6 m off a centre pose, seen from 2 .. 5 poses around it
    centre = rng.integers(0, n_poses, size=n_lm)
    ang, dist = rng.uniform(-np.pi, np.pi, size=n_lm), rng.uniform(3.0, 6.0, size=n_lm)
    Lm = xy[centre] + dist[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    po, lo = [], []
    for l in range(n_lm):
        seen = np.unique(np.clip(centre[l] + rng.integers(-window, window + 1, size=rng.integers(views[0], views[1] + 1)), 0, n_poses - 1))
        if seen.size < 2:
            seen = np.unique(np.clip([centre[l] - 1, centre[l], centre[l] + 1], 0, n_poses - 1))[:2]
        po.append(seen)
        lo.append(np.full(seen.size, l))
    po, lo = np.concatenate(po), np.concatenate(lo)
    d = Lm[lo] - xy[po]
    z_obs = np.stack([np.hypot(d[:, 0], d[:, 1]), np.arctan2(d[:, 1], d[:, 0]) - th[po]], axis=1)
    z_obs += rng.normal(0, 1, size=z_obs.shape) * np.array([0.05, 0.01])
    z_obs[:, 1] = np.fmod(z_obs[:, 1], 2 * np.pi)
    obs_info = np.tile(np.diag([400.0, 10000.0]), (po.size, 1, 1))
    # global edge order: by the later pose of the edge, odometry before the observations made there
    t_all = np.concatenate([np.maximum(oi, oj), po])
    order = np.argsort(t_all, kind="stable")
    seq = np.empty(order.size, dtype=np.int64)
    seq[order] = np.arange(order.size)
    # initial estimate: dead reckoning, landmarks from their first observation (in the global order)
    est = np.zeros((n_poses, 3))
    for i in range(n_poses - 1):
        c, s_ = np.cos(est[i, 2]), np.sin(est[i, 2])
        est[i + 1] = [est[i, 0] + c * z_odo[i, 0] - s_ * z_odo[i, 1], est[i, 1] + s_ * z_odo[i, 0] + c * z_odo[i, 1],
                      np.fmod(est[i, 2] + z_odo[i, 2], 2 * np.pi)]
    first = np.full(n_lm, -1)
    for k in np.argsort(seq[oi.size:], kind="stable"):
        if first[lo[k]] < 0:
            first[lo[k]] = k
    b = est[po[first], 2] + z_obs[first, 1]
    lm_est = est[po[first], :2] + z_obs[first, :1] * np.stack([np.cos(b), np.sin(b)], axis=1)
    dim = np.empty(nv, dtype=np.int32)
    dim[pose_id], dim[lm_id] = 3, 2
    base = np.zeros(nv + 1, dtype=np.int64)
    np.cumsum(dim, out=base[1:])
    state = np.empty(base[-1])
    state[base[pose_id][:, None] + np.arange(3)] = est
    state[base[lm_id][:, None] + np.arange(2)] = lm_est
    f = lambda a: a.astype(np.float64)
    return Problem(name=name, dim=dim, state=state, unary_vertex=0, pose_id=pose_id, lm_id=lm_id,
                   odo=np.concatenate([f(pose_id[oi])[:, None], f(pose_id[oj])[:, None], z_odo], axis=1), odo_info=odo_info,
                   odo_seq=seq[:oi.size].copy(),
                   obs=np.concatenate([f(pose_id[po])[:, None], f(lm_id[lo])[:, None], z_obs], axis=1), obs_info=obs_info,
                   obs_seq=seq[oi.size:].copy(), truth=dict(poses=P, landmarks=Lm))


def slam3d_problem(n_poses=40, n_lm=60, seed=71, interleave=False, name="slam3d", views=(2, 5), window=5, hubs=0):
    """3D landmark SLAM: a trajectory along a helix with noisy odometry (CEdgePose3D) and n_poses // 5 loop closures,
    landmarks each seen from views[0] .. views[1] nearby poses as noisy XYZ points in the pose's frame
    (CEdgePoseLandmark3D) -- two edge groups, (6, 6, 6) and (6, 3, 3), over the same vertices. The measurements come from a
    ground truth, the initial estimate is what a reader of the edge list builds: dead reckoning along the odometry, every
    landmark where its first observation sees it (t + R z). interleave=True shuffles the vertex ids (vertex 0 stays the
    first pose, which carries the unary factor), so that landmarks sit between the poses and about half of the
    pose-landmark blocks are stored transposed. hubs > 0: landmark 0 is seen from `hubs` poses more and the middle pose
    sees `hubs` landmarks more (vertices of both widths with a degree the sequential assembly kernel leaves to the wave
    kernel). The edges are in the order of an incremental run: each when its later pose arrives.
    Returns Problem(dim, state (flat, laid out by dim), odo (m, 8) i j t axis-angle, odo_info, odo_seq, obs (k, 5) pose
    landmark x y z, obs_info, obs_seq, pose_id, lm_id, truth, unary_vertex)."""
    from scipy.spatial.transform import Rotation
    from .formats import se3_plus
    rng = np.random.default_rng(seed)
    nv = n_poses + n_lm
    if interleave:
        ids = 1 + rng.permutation(nv - 1)
        pose_id, lm_id = np.concatenate([[0], ids[:n_poses - 1]]), ids[n_poses - 1:]
    else:
        pose_id, lm_id = np.arange(n_poses), n_poses + np.arange(n_lm)
    # ground truth: a helix of radius 5 rising 0.15 per step, flown without turning into the curve: the attitude only
    # wobbles by about 0.1 rad, so that the rotation between ANY two poses stays small. (CEdgePose3D pairs the Jacobian of
    # the expectation with the error log(R(z) R(e)^T), SE3_Types.h:264-286, which is the error's own Jacobian only up to
    # the rotation between the two poses; with loop closures across a quarter turn of a turning trajectory Gauss-Newton
    # on that linearization does not settle.) Pose 0 is the origin (the reader starts the first vertex there)
    a = 0.25 * np.arange(n_poses)
    pos = np.stack([5 * np.cos(a) - 5, 5 * np.sin(a), 0.15 * np.arange(n_poses)], axis=1)
    Rw = Rotation.from_euler("ZYX", np.stack([0.12 * np.sin(0.6 * a), 0.08 * np.sin(0.4 * a + 1), 0.05 * np.sin(0.8 * a)], axis=1))
    R0i = Rw[0].inv()
    pos, Rw = R0i.apply(pos - pos[0]), R0i * Rw
    P = np.concatenate([pos, Rw.as_rotvec()], axis=1)

    def rel(i, j):  # pose j in the frame of pose i
        Ri = Rw[i].inv()
        return np.concatenate([Ri.apply(pos[j] - pos[i]), (Ri * Rw[j]).as_rotvec()], axis=1)

    oi = np.arange(n_poses - 1)
    oj = oi + 1
    lc = np.sort(np.stack([rng.choice(n_poses, size=2, replace=False) for _ in range(n_poses // 5)]), axis=1)
    oi, oj = np.concatenate([oi, lc[:, 0]]), np.concatenate([oj, lc[:, 1]])
    # odometry along the chain, loop closures from a ten times finer sensor: dead reckoning misses the closures by many
    # of their sigmas while staying inside Gauss-Newton's basin
    chain = (np.arange(oi.size) < n_poses - 1)[:, None]
    sig = np.where(chain, np.array([0.02] * 3 + [0.004] * 3), np.array([0.002] * 3 + [0.0004] * 3))
    z_odo = rel(oi, oj)
    z_odo[:, :3] += rng.normal(0, 1, size=(oi.size, 3)) * sig[:, :3]
    z_odo[:, 3:] = (Rotation.from_rotvec(z_odo[:, 3:]) * Rotation.from_rotvec(rng.normal(0, 1, size=(oi.size, 3)) * sig[:, 3:])).as_rotvec()
    odo_info = np.zeros((oi.size, 6, 6))
    odo_info[:, np.arange(6), np.arange(6)] = 1.0 / sig ** 2
    # landmarks: 2 .. 5 m off a centre pose, seen from a few poses around it
    centre = rng.integers(0, n_poses, size=n_lm)
    off = rng.normal(size=(n_lm, 3))
    Lm = pos[centre] + off / np.linalg.norm(off, axis=1, keepdims=True) * rng.uniform(2.0, 5.0, size=(n_lm, 1))
    po, lo = [], []
    for l in range(n_lm):
        seen = np.unique(np.clip(centre[l] + rng.integers(-window, window + 1, size=rng.integers(views[0], views[1] + 1)), 0, n_poses - 1))
        if seen.size < 2:
            seen = np.unique(np.clip([centre[l] - 1, centre[l], centre[l] + 1], 0, n_poses - 1))[:2]
        po.append(seen)
        lo.append(np.full(seen.size, l))
    if hubs:
        extra = np.setdiff1d(np.arange(n_poses), po[0])[:hubs]            # landmark 0: `hubs` more poses
        po.append(extra)
        lo.append(np.zeros(extra.size, dtype=np.int64))
        mid = n_poses // 2
        more = np.array([l for l in range(1, n_lm) if mid not in po[l]][:hubs])   # pose mid: `hubs` more landmarks
        po.append(np.full(more.size, mid))
        lo.append(more)
    po, lo = np.concatenate(po).astype(np.int64), np.concatenate(lo).astype(np.int64)
    sig_obs = np.array([0.02, 0.03, 0.05])
    z_obs = Rw[po].inv().apply(Lm[lo] - pos[po]) + rng.normal(0, 1, size=(po.size, 3)) * sig_obs
    obs_info = np.tile(np.diag(1.0 / sig_obs ** 2), (po.size, 1, 1))
    # global edge order: by the later pose of the edge, odometry before the observations made there
    t_all = np.concatenate([np.maximum(oi, oj), po])
    order = np.argsort(t_all, kind="stable")
    seq = np.empty(order.size, dtype=np.int64)
    seq[order] = np.arange(order.size)
    # initial estimate: dead reckoning, landmarks from their first observation (in the global order)
    est = np.zeros((n_poses, 6))
    for i in range(n_poses - 1):
        est[i + 1] = se3_plus(est[i:i + 1], z_odo[i:i + 1])[0]
    first = np.full(n_lm, -1)
    for k in np.argsort(seq[oi.size:], kind="stable"):
        if first[lo[k]] < 0:
            first[lo[k]] = k
    lm_est = np.stack([est[po[k], :3] + Rotation.from_rotvec(est[po[k], 3:]).apply(z_obs[k]) for k in first])
    dim = np.empty(nv, dtype=np.int32)
    dim[pose_id], dim[lm_id] = 6, 3
    base = np.zeros(nv + 1, dtype=np.int64)
    np.cumsum(dim, out=base[1:])
    state = np.empty(base[-1])
    state[base[pose_id][:, None] + np.arange(6)] = est
    state[base[lm_id][:, None] + np.arange(3)] = lm_est
    f = lambda a: a.astype(np.float64)
    return Problem(name=name, dim=dim, state=state, unary_vertex=0, pose_id=pose_id, lm_id=lm_id,
                   odo=np.concatenate([f(pose_id[oi])[:, None], f(pose_id[oj])[:, None], z_odo], axis=1), odo_info=odo_info,
                   odo_seq=seq[:oi.size].copy(),
                   obs=np.concatenate([f(pose_id[po])[:, None], f(lm_id[lo])[:, None], z_obs], axis=1), obs_info=obs_info,
                   obs_seq=seq[oi.size:].copy(), truth=dict(poses=P, landmarks=Lm))


def landmark3d_problem(n_poses=40, n_lm=60, seed=72, name="lm3d_small"):
    """the (6, 3, 3) observations of a slam3d_problem alone, linearized at its initial estimate, as ONE homogeneous edge
    group for the one-group entry points (damped: without the odometry only the observations hold the poses)"""
    from .formats import slam3d_linearize
    p = slam3d_problem(n_poses, n_lm, seed, name=name)
    g = slam3d_linearize(p.dim, p.state, p.odo, p.odo_info, p.obs, p.obs_info)[1]
    g["name"], g["damping"] = name, 1e-2
    return g


# ------------------------------------------------------------------------------------------------
# range-only constant-velocity SLAM (ROCV): receivers [p | v] (6) + transmitters (3); constant-velocity edges (6, 6, 6),
# ranges (6, 3, 1), transmitter priors: unary (3, 3)
# ------------------------------------------------------------------------------------------------
def rocv_problem(n_receivers=40, n_transmitters=5, seed=81, interleave=False, n_ranges=4, hub=0, name="rocv"):
    """Range-only SLAM with a constant-velocity motion model (src/slam_app/SolveROCVImpl.cpp): a receiver flies a smooth
    rising curve (about 2 m/s, a time step of about 1 s with jitter), its true velocity turning with the curve -- the
    noise of the constant-velocity edges CEdgeConstVelocity3D --; every receiver ranges a random subset of n_ranges
    transmitters (CEdgePosVel_Landmark3D, sigma 0.05); the transmitters stand around the curve at different heights, start
    0.3 m off their true places and are held there by priors (CEdgeLandmark3DPrior; full 3x3 information matrices).
    Vertex ids: half of the transmitters below the receivers' ids and half above, so that range blocks appear in both
    orientations; interleave=True scatters the transmitters' ids among the receivers'. hub > 0: the middle receiver ranges EVERY transmitter `hub` times
    (a 6-wide vertex beyond the sequential assembly kernel's 24 sources; a transmitter passes them once more than 24
    receivers range it). Receivers start at the truth + noise (0.2 m, 0.1 m/s) and have a ROCV:RECEIVER line, except
    every eighth, which starts where CConstVelocity_Initializer puts it: (p + v dt, v) of its predecessor. The edges are in
    the order of an incremental run -- the first half of the priors, then per receiver its constant-velocity edge and its
    ranges, then the other priors.
    Returns Problem(dim, state (flat, laid out by dim), cv (m, 3) i j dt, cv_info, cv_seq, rng (k, 3) receiver transmitter
    range, rng_info (k,), rng_seq, pri (p,), pri_info, pri_seq, explicit, recv_id, tx_id, truth, unary_vertex = -1)."""
    rng = np.random.default_rng(seed)
    R, T = n_receivers, n_transmitters
    nv = R + T
    if interleave:
        ids = rng.permutation(nv)   # (receiver ids ascend along the chain: the parser drops a ROCV:DELTA_TIME line with i > j)
        recv_id, tx_id = np.sort(ids[:R]), ids[R:]
    else:
        lo = T // 2
        recv_id, tx_id = lo + np.arange(R), np.concatenate([np.arange(lo), lo + R + np.arange(T - lo)])
    dt = 1.0 + rng.uniform(-0.05, 0.05, size=R - 1)
    t = np.concatenate([[0.0], np.cumsum(dt)])
    w = 0.2
    pos = np.stack([10 * np.cos(w * t), 10 * np.sin(w * t), 0.3 * t], axis=1)
    vel = np.stack([-10 * w * np.sin(w * t), 10 * w * np.cos(w * t), np.full(R, 0.3)], axis=1)
    X = np.concatenate([pos, vel], axis=1)
    ang = 2 * np.pi * (np.arange(T) + 0.3) / T
    Tx = np.stack([18 * np.cos(ang), 18 * np.sin(ang), np.where(np.arange(T) % 2 == 0, -4.0, 12.0) + rng.uniform(-1, 1, size=T)], axis=1)
    # constant-velocity edges along the chain: dp = 0.5 a dt^2 ~ 0.2, dv = a dt ~ 0.4 with a = 10 w^2
    cv_info = np.tile(np.diag([1 / 0.2 ** 2] * 3 + [1 / 0.4 ** 2] * 3), (R - 1, 1, 1))
    nr = min(n_ranges, T)
    rr, rt = [], []
    for i in range(R):
        seen = np.sort(rng.choice(T, size=nr, replace=False))
        rr.append(np.full(nr, i))
        rt.append(seen)
        if hub and i == R // 2:
            rr.append(np.full(hub * T, i))
            rt.append(np.tile(np.arange(T), hub))
    rr, rt = np.concatenate(rr).astype(np.int64), np.concatenate(rt).astype(np.int64)
    z = np.linalg.norm(pos[rr] - Tx[rt], axis=1) + rng.normal(0, 0.05, size=rr.size)
    rng_info = np.full(rr.size, 1 / 0.05 ** 2)
    A = rng.normal(size=(T, 3, 3)) * 0.3 + np.eye(3)
    pri_info = A @ A.transpose(0, 2, 1) / 0.3 ** 2
    # global edge order
    first = np.arange(T) < (T + 1) // 2
    t_cv, t_rng = 1.0 + np.arange(1, R), 1.0 + rr + 0.5
    t_pri = np.where(first, 0.0, R + 2.0)
    order = np.argsort(np.concatenate([t_cv, t_rng, t_pri]), kind="stable")
    seq = np.empty(order.size, dtype=np.int64)
    seq[order] = np.arange(order.size)
    # initial estimate
    est = X + np.concatenate([rng.normal(0, 0.2, size=(R, 3)), rng.normal(0, 0.1, size=(R, 3))], axis=1)
    listed = np.arange(R) % 8 != 5
    for i in np.flatnonzero(~listed):
        est[i] = np.concatenate([est[i - 1, :3] + est[i - 1, 3:] * dt[i - 1], est[i - 1, 3:]])
    d = rng.normal(size=(T, 3))
    tx_est = Tx + 0.3 * d / np.linalg.norm(d, axis=1, keepdims=True)
    dim = np.empty(nv, dtype=np.int32)
    dim[recv_id], dim[tx_id] = 6, 3
    base = np.zeros(nv + 1, dtype=np.int64)
    np.cumsum(dim, out=base[1:])
    state = np.empty(base[-1])
    state[base[recv_id][:, None] + np.arange(6)] = est
    state[base[tx_id][:, None] + np.arange(3)] = tx_est
    explicit = np.ones(nv, dtype=bool)
    explicit[recv_id[~listed]] = False
    f = lambda a: a.astype(np.float64)
    m = R - 1
    return Problem(name=name, dim=dim, state=state, unary_vertex=-1, recv_id=recv_id, tx_id=tx_id, explicit=explicit,
                   cv=np.stack([f(recv_id[:-1]), f(recv_id[1:]), dt], axis=1), cv_info=cv_info, cv_seq=seq[:m].copy(),
                   rng=np.stack([f(recv_id[rr]), f(tx_id[rt]), z], axis=1), rng_info=rng_info, rng_seq=seq[m:m + rr.size].copy(),
                   pri=tx_id.astype(np.int64), pri_info=pri_info, pri_seq=seq[m + rr.size:].copy(),
                   truth=dict(receivers=X, transmitters=Tx))


# ------------------------------------------------------------------------------------------------
# stereo bundle adjustment: cameras CVertexSCam (6) + points (3), 3-d residuals (u, v, u_right), CEdgeP2SC3D
# ------------------------------------------------------------------------------------------------
def stereo_problem(nc=6, npts=40, seed=16, interleave=False, views=(2, 6), hubs=False, name="stereo"):
    """nc stereo cameras on a circle of radius 10 looking at the origin (scene depth about 10, baseline 0.5 = 1/20 of it),
    npts points in a cube, each seen by views[0] .. views[1] distinct cameras; fx 500, fy 505, c = (320, 240), the
    distortion d = 0.1 on every odd camera and 0 on the even ones. hubs: point 0 is seen by ALL cameras and camera 0 sees
    30 points more (vertices of both widths beyond the 24 entries the sequential assembly kernel takes).
    interleave=True shuffles the vertex ids. The measurements come from the ground truth + pixel noise (sigma 0.5 / 0.5 /
    0.7, information its inverse square), the estimate is the truth disturbed (cameras 0.03 / 0.004 rad, points 0.05), so
    that Levenberg-Marquardt has work to do. Returns the (6, 3, 3) group linearized at the estimate (formats.
    stereo_linearize: measurements = expectation + r) with geometry = the states (stereo_states)."""
    from scipy.spatial.transform import Rotation
    from .formats import stereo_expectation, stereo_linearize
    rng = np.random.default_rng(seed)
    k = rng.integers(views[0], min(views[1], nc) + 1, size=npts)
    cam_of = np.concatenate([np.sort(rng.choice(nc, size=kk, replace=False)) for kk in k])
    pt_of = np.repeat(np.arange(npts, dtype=np.int64), k)
    if hubs:
        more_c = np.setdiff1d(np.arange(nc), cam_of[pt_of == 0])                 # point 0: every camera
        more_p = np.array([j for j in range(1, npts) if 0 not in cam_of[pt_of == j]][:30])   # camera 0: 30 points more
        cam_of = np.concatenate([cam_of, more_c, np.zeros(more_p.size, dtype=np.int64)])
        pt_of = np.concatenate([pt_of, np.zeros(more_c.size, dtype=np.int64), more_p])
    nobs = cam_of.size
    th = 2 * np.pi * np.arange(nc) / nc
    C = np.stack([10 * np.cos(th), 10 * np.sin(th), 0.5 * np.sin(3 * th)], axis=1)
    z = -C / np.linalg.norm(C, axis=1, keepdims=True)
    x = np.cross(np.array([0.0, 0.0, 1.0])[None, :], z)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    R = np.stack([x, np.cross(z, x), z], axis=1)  # rows = camera axes (world -> camera)
    cams = np.concatenate([-np.einsum("cij,cj->ci", R, C), Rotation.from_matrix(R).as_rotvec()], axis=1)
    intr = np.tile(np.array([500.0, 505.0, 320.0, 240.0, 0.0, 0.5]), (nc, 1))
    intr[1::2, 4] = 0.1
    X = rng.uniform(-2, 2, size=(npts, 3))
    sig = np.array([0.5, 0.5, 0.7])
    meas = stereo_expectation(cams[cam_of], intr[cam_of], X[pt_of]) + rng.normal(0, 1, size=(nobs, 3)) * sig
    info = np.tile(np.diag(1.0 / sig ** 2), (nobs, 1, 1))
    est_c = np.concatenate([cams[:, :3] + rng.normal(0, 0.03, size=(nc, 3)),
                            (Rotation.from_rotvec(cams[:, 3:]) * Rotation.from_rotvec(rng.normal(0, 0.004, size=(nc, 3)))).as_rotvec()], axis=1)
    est_p = X + rng.normal(0, 0.05, size=X.shape)
    nv = nc + npts
    if interleave:
        perm = rng.permutation(nv)
        cam_id, pt_id = perm[:nc], perm[nc:]
    else:
        cam_id, pt_id = np.arange(nc), nc + np.arange(npts)
    f = lambda a: a.astype(np.float64)
    obs = np.concatenate([f(cam_of)[:, None], f(pt_of)[:, None], meas], axis=1)
    prob = stereo_linearize(est_c, intr, est_p, obs, cam_id, pt_id, info)
    J0, J1, Om = prob.J0.reshape(nobs, 6, 3), prob.J1.reshape(nobs, 3, 3), info
    h0 = np.einsum("eci,eij,ecj->ec", J0, Om, J0).max()
    h1 = np.einsum("eci,eij,ecj->ec", J1, Om, J1).max()
    prob.update(name=name, damping=1e-3 * float(max(h0, h1)), nc=nc, npts=npts,
                geometry=dict(cams=est_c, intr=intr, points=est_p, obs=obs, info=info, cam_of=cam_of, pt_of=pt_of,
                              cam_id=cam_id, pt_id=pt_id, truth=dict(cams=cams, points=X)))
    return prob


def stereo_states(prob):
    """The scene of a stereo_problem as input of spp_ba_stereo_linearize_device, like ba_states: dict(cams (nc,6), intr
    (nc,6) fx fy cx cy d b, points (np,3), meas (no,3) = expectation + the problem's residual, cam_of, pt_of int32,
    cam_dxoff, pt_dxoff int64: scalar offset of every vertex in the solution vector)."""
    g = prob.geometry
    base = np.zeros(prob.dim.size + 1, dtype=np.int64)
    np.cumsum(prob.dim, out=base[1:])
    return dict(cams=g["cams"].copy(), intr=g["intr"].copy(), points=g["points"].copy(), meas=g["obs"][:, 2:5].copy(),
                cam_of=g["cam_of"].astype(np.int32), pt_of=g["pt_of"].astype(np.int32),
                cam_dxoff=base[g["cam_id"]].copy(), pt_dxoff=base[g["pt_id"]].copy())


# ------------------------------------------------------------------------------------------------
# Sim(3) bundle adjustment: cameras (7: [t | w | s] in sim(3)) + points (3), CEdgeP2C_XYZ_Sim3_G observations
# ------------------------------------------------------------------------------------------------
def sim3_problem(nc=6, npts=40, seed=26, interleave=False, views=(2, 6), hubs=False, name="sim3"):
    """nc Sim(3) cameras on a ring of radius 10 around a point cloud, looking at the origin, with scales e^s, s uniform in
    [-0.3, 0.3] (a camera is T = (R, centre, e^s), x = T^-1 X: its frame measures the scene in units of e^s); npts points in
    a cube, each seen by views[0] .. views[1] distinct cameras; fx 500, fy 505, c = (320, 240), d = 0.1 on every odd camera
    (divided by 0.5 fx fy in the projection). hubs: point 0 is seen by ALL cameras and camera 0 sees ALL points
    (vertices of both widths beyond the 24 entries the sequential assembly kernel takes). interleave=True shuffles the
    vertex ids. Measurements: the truth's projection + pixel noise (sigma 0.5, information its inverse square); the
    estimate is the truth disturbed -- cameras by T Exp(d) with d ~ (0.03, 0.004 rad, 0.01), points by 0.05. Returns the
    (7, 3, 2) group linearized at the estimate (formats.sim3_ba_linearize) with geometry = the states (sim3_states)."""
    from scipy.spatial.transform import Rotation
    from .formats import sim3_ba_linearize, sim3_expectation, sim3_from_trs, sim3_plus, sim3_to_trs
    rng = np.random.default_rng(seed)
    k = rng.integers(views[0], min(views[1], nc) + 1, size=npts)
    cam_of = np.concatenate([np.sort(rng.choice(nc, size=kk, replace=False)) for kk in k])
    pt_of = np.repeat(np.arange(npts, dtype=np.int64), k)
    if hubs:
        more_c = np.setdiff1d(np.arange(nc), cam_of[pt_of == 0])                         # point 0: every camera
        more_p = np.array([j for j in range(1, npts) if 0 not in cam_of[pt_of == j]])    # camera 0: every point
        cam_of = np.concatenate([cam_of, more_c, np.zeros(more_p.size, dtype=np.int64)])
        pt_of = np.concatenate([pt_of, np.zeros(more_c.size, dtype=np.int64), more_p])
    nobs = cam_of.size
    th = 2 * np.pi * np.arange(nc) / nc
    C = np.stack([10 * np.cos(th), 10 * np.sin(th), 0.5 * np.sin(3 * th)], axis=1)
    z = -C / np.linalg.norm(C, axis=1, keepdims=True)
    x = np.cross(np.array([0.0, 0.0, 1.0])[None, :], z)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    R = np.stack([x, np.cross(z, x), z], axis=1)  # rows = camera axes (world -> camera); the pose holds its transpose
    scale = np.exp(rng.uniform(-0.3, 0.3, size=nc))
    cams = sim3_from_trs(np.concatenate([C, Rotation.from_matrix(R.transpose(0, 2, 1)).as_rotvec(), scale[:, None]], axis=1))
    intr = np.tile(np.array([500.0, 505.0, 320.0, 240.0, 0.0]), (nc, 1))
    intr[1::2, 4] = 0.1
    X = rng.uniform(-2, 2, size=(npts, 3))
    sig = 0.5
    meas = sim3_expectation(cams[cam_of], intr[cam_of], X[pt_of])[0] + rng.normal(0, sig, size=(nobs, 2))
    info = np.tile(np.eye(2) / sig ** 2, (nobs, 1, 1))
    est_c = sim3_plus(cams, rng.normal(0, 1, size=(nc, 7)) * np.array([0.03] * 3 + [0.004] * 3 + [0.01]))
    est_p = X + rng.normal(0, 0.05, size=X.shape)
    nv = nc + npts
    if interleave:
        perm = rng.permutation(nv)
        cam_id, pt_id = perm[:nc], perm[nc:]
    else:
        cam_id, pt_id = np.arange(nc), nc + np.arange(npts)
    f = lambda a: a.astype(np.float64)
    obs = np.concatenate([f(cam_of)[:, None], f(pt_of)[:, None], meas], axis=1)
    prob = sim3_ba_linearize(est_c, intr, est_p, obs, cam_id, pt_id, info)
    J0, J1 = prob.J0.reshape(nobs, 7, 2), prob.J1.reshape(nobs, 3, 2)
    h0 = np.einsum("eci,eij,ecj->ec", J0, info, J0).max()
    h1 = np.einsum("eci,eij,ecj->ec", J1, info, J1).max()
    prob.update(name=name, damping=1e-3 * float(max(h0, h1)), nc=nc, npts=npts,
                geometry=dict(cams=est_c, cams_trs=sim3_to_trs(est_c), intr=intr, points=est_p, obs=obs, info=info, cam_of=cam_of,
                              pt_of=pt_of, cam_id=cam_id, pt_id=pt_id, truth=dict(cams=cams, points=X)))
    return prob


def sim3_states(prob):
    """The scene of a sim3_problem as input of spp_sim3_ba_linearize_device, like stereo_states: dict(cams (nc,7), intr
    (nc,5), points (np,3), meas (no,2), cam_of, pt_of int32, cam_dxoff, pt_dxoff int64: scalar offset of every vertex in
    the solution vector)."""
    g = prob.geometry
    base = np.zeros(prob.dim.size + 1, dtype=np.int64)
    np.cumsum(prob.dim, out=base[1:])
    return dict(cams=g["cams"].copy(), intr=g["intr"].copy(), points=g["points"].copy(), meas=g["obs"][:, 2:4].copy(),
                cam_of=g["cam_of"].astype(np.int32), pt_of=g["pt_of"].astype(np.int32),
                cam_dxoff=base[g["cam_id"]].copy(), pt_dxoff=base[g["pt_id"]].copy())


# ------------------------------------------------------------------------------------------------
# self-calibrating bundle adjustment: cameras (6) + points (3) + intrinsics vertices (5, stored 6 wide), ternary
# CEdgeP2CI3D observations with 2-d residuals
# ------------------------------------------------------------------------------------------------
def bai_problem(ni=1, nc=3, npts=12, seed=20, views=(2, 3), layout="first", name="bai"):
    """nc cameras on a circle of radius 10 looking at the origin, camera j using intrinsics vertex j % ni (the cameras
    alternate between them); intrinsics vertex i: fx 500 + 20 i, fy 505 + 20 i (fx != fy), c = (320 + 5 i, 240 - 3 i), kappa
    = 0.02 (0.5 (fx + fy)) / 70^2 -- the distortion reaches 2 % at 70 pixels from the centre, the edge of what the cameras see
    of the scene; npts points in the cube [-1, 1]^3, each
    seen by views[0] .. views[1] distinct cameras. layout: where the intrinsics vertices get their ids -- "first" (0 ..
    ni - 1, cameras and points after them: ids the reference application accepts), "last", or "interleaved" (all ids
    shuffled). Measurements: the truth + pixel noise of sigma 0.5 (information 4 I). Estimate: the truth disturbed by 0.03 /
    0.004 rad (cameras), 0.05 (points), 2 / 2 / 1 / 1 pixels on fx fy cx cy and 10 % of kappa: the host float64
    Levenberg-Marquardt loop brings chi2 monotonically below 0.05 of its initial value within 5 iterations
    (tests/test_bai_host.py). Returns the ternary group linearized at the estimate (formats.bai_linearize) with geometry
    = the states."""
    from scipy.spatial.transform import Rotation
    from .formats import bai_expectation, bai_linearize
    rng = np.random.default_rng(seed)
    k = rng.integers(views[0], min(views[1], nc) + 1, size=npts)
    cam_of = np.concatenate([np.sort(rng.choice(nc, size=kk, replace=False)) for kk in k])
    pt_of = np.repeat(np.arange(npts, dtype=np.int64), k)
    intr_of = cam_of % ni
    nobs = cam_of.size
    th = 2 * np.pi * np.arange(nc) / nc
    C = np.stack([10 * np.cos(th), 10 * np.sin(th), 0.5 * np.sin(3 * th)], axis=1)
    z = -C / np.linalg.norm(C, axis=1, keepdims=True)
    x = np.cross(np.array([0.0, 0.0, 1.0])[None, :], z)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    R = np.stack([x, np.cross(z, x), z], axis=1)  # rows = camera axes (world -> camera)
    cams = np.concatenate([-np.einsum("cij,cj->ci", R, C), Rotation.from_matrix(R).as_rotvec()], axis=1)
    i = np.arange(ni, dtype=np.float64)
    intr = np.stack([500 + 20 * i, 505 + 20 * i, 320 + 5 * i, 240 - 3 * i, np.zeros(ni)], axis=1)
    intr[:, 4] = 0.02 * (0.5 * (intr[:, 0] + intr[:, 1])) / 70.0 ** 2
    X = rng.uniform(-1, 1, size=(npts, 3))
    meas = bai_expectation(cams[cam_of], intr[intr_of], X[pt_of]) + rng.normal(0, 0.5, size=(nobs, 2))
    info = np.tile(4.0 * np.eye(2), (nobs, 1, 1))
    est_c = np.concatenate([cams[:, :3] + rng.normal(0, 0.03, size=(nc, 3)),
                            (Rotation.from_rotvec(cams[:, 3:]) * Rotation.from_rotvec(rng.normal(0, 0.004, size=(nc, 3)))).as_rotvec()], axis=1)
    est_p = X + rng.normal(0, 0.05, size=X.shape)
    est_i = intr + rng.normal(0, 1, size=intr.shape) * np.array([2.0, 2.0, 1.0, 1.0, 0.0])
    est_i[:, 4] = intr[:, 4] * (1 + 0.1 * rng.normal(0, 1, size=ni))
    nv = ni + nc + npts
    if layout == "first":
        intr_id, cam_id, pt_id = np.arange(ni), ni + np.arange(nc), ni + nc + np.arange(npts)
    elif layout == "last":
        cam_id, pt_id, intr_id = np.arange(nc), nc + np.arange(npts), nc + npts + np.arange(ni)
    else:
        perm = rng.permutation(nv)
        intr_id, cam_id, pt_id = perm[:ni], perm[ni:ni + nc], perm[ni + nc:]
    f = lambda a: a.astype(np.float64)
    obs = np.concatenate([f(cam_of)[:, None], f(pt_of)[:, None], f(intr_of)[:, None], meas], axis=1)
    prob = bai_linearize(est_c, est_i, est_p, obs, cam_id, pt_id, intr_id, info)
    prob.update(name=name, ni=ni, nc=nc, npts=npts,
                geometry=dict(cams=est_c, intr=est_i, points=est_p, obs=obs, info=info, cam_of=cam_of, pt_of=pt_of, intr_of=intr_of,
                              cam_id=cam_id, pt_id=pt_id, intr_id=intr_id, truth=dict(cams=cams, intr=intr, points=X)))
    return prob


def bai_tiny(layout="first"):
    """1 intrinsics vertex, 3 cameras, 12 points"""
    return bai_problem(1, 3, 12, 20, views=(2, 3), layout=layout, name="bai_tiny")


def bai_small(layout="first"):
    """2 intrinsics vertices, 6 cameras alternating between them, 40 points seen by 2 .. 6 cameras: a point has two (point,
    intrinsics) blocks"""
    return bai_problem(2, 6, 40, 21, views=(2, 6), layout=layout, name="bai_small")


def bai_hub(layout="first"):
    """1 intrinsics vertex, 40 cameras, 3000 points seen by 2 .. 6 cameras: the intrinsics' block of S is split over several
    work items of the Schur plan (n_multi >= 1), its H22 and its blocks against the cameras go through the hub reduction"""
    return bai_problem(1, 40, 3000, 22, views=(2, 6), layout=layout, name="bai_hub")


def bai_states(prob):
    """The scene of a bai_problem as input of spp_ba_intrinsics_linearize_device: dict(cams (nc,6), intr (ni,5), points
    (np,3), meas (no,2), cam_of, pt_of, intr_of int32, cam_dxoff, pt_dxoff, intr_dxoff int64: scalar offset of every vertex in
    the padded solution vector)."""
    g = prob.geometry
    base = np.zeros(prob.dim.size + 1, dtype=np.int64)
    np.cumsum(prob.dim, out=base[1:])
    return dict(cams=g["cams"].copy(), intr=g["intr"].copy(), points=g["points"].copy(), meas=g["obs"][:, 3:5].copy(),
                cam_of=g["cam_of"].astype(np.int32), pt_of=g["pt_of"].astype(np.int32), intr_of=g["intr_of"].astype(np.int32),
                cam_dxoff=base[g["cam_id"]].copy(), pt_dxoff=base[g["pt_id"]].copy(), intr_dxoff=base[g["intr_id"]].copy())


def pose_graph_states(prob):
    """The same pose graph as states + measurements in the REFERENCE's parameterization, as input of
    spp_se2_/se3_linearize_device: poses (n, 3) x y theta or (n, 6) [t | axis-angle] at the noisy estimate,
    meas (ne, 3 or 6) = relative pose of the ground truth + sensor noise, v0 / v1 int32."""
    g = prob.geometry
    if g["kind"] == "se2":
        return dict(dof=3, poses=g["poses"], meas=g["meas"], v0=prob.v0.astype(np.int32), v1=prob.v1.astype(np.int32))
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(g["seed"] + 1)
    Rt, Re = Rotation.from_matrix(g["R"]), Rotation.from_matrix(g["Re"])   # from_matrix projects Re onto SO(3)
    v0, v1 = prob.v0, prob.v1
    zt = Rt[v0].inv().apply(g["t"][v1] - g["t"][v0]) + rng.normal(0, 0.05, size=(v0.size, 3))
    zr = (Rt[v0].inv() * Rt[v1] * Rotation.from_rotvec(rng.normal(0, 0.01, size=(v0.size, 3)))).as_rotvec()
    return dict(dof=6, poses=np.concatenate([g["te"], Re.as_rotvec()], axis=1), meas=np.concatenate([zt, zr], axis=1),
                v0=v0.astype(np.int32), v1=v1.astype(np.int32))


# ------------------------------------------------------------------------------------------------
# the five BASELINE.json configs + small variants for fast tests
# ------------------------------------------------------------------------------------------------
CONFIGS = {
    "manhattan3500": lambda: se2_problem(3500, 2099, 1234),
    "sphere2500": lambda: se3_problem(50, 50, 2500),
    "ladybug49": lambda: ba_problem(49, 7776, 31843, 49, heavy_tail=False, spread=0.06, name="ladybug49"),
    "venice871": lambda: ba_problem(871, 530304, 2838740, 871, heavy_tail=True, name="venice871"),
    "synthetic10k": lambda: ba_problem(10000, 2000000, 10000000, 10000, heavy_tail=False, spread=0.0005, name="synthetic10k"),
    # small cases (seconds on the CPU oracle)
    "ba_tiny": lambda: ba_problem(7, 40, 150, 7, heavy_tail=True, spread=0.5, name="ba_tiny"),
    "ba_small": lambda: ba_problem(30, 1500, 7000, 30, heavy_tail=True, spread=0.2, name="ba_small"),
    "ba_interleaved": lambda: ba_problem(25, 900, 4000, 25, heavy_tail=True, interleave=True, spread=0.3, name="ba_interleaved"),
    "ba_medium": lambda: ba_problem(150, 20000, 100000, 150, heavy_tail=True, name="ba_medium"),
    # a long camera trajectory: every point is seen from a narrow window of cameras, the reduced camera
    # system is banded (the shape of BASELINE config 5 at a size the CPU reference finishes in seconds)
    "ba_banded": lambda: ba_problem(600, 30000, 150000, 600, heavy_tail=False, spread=0.01, name="ba_banded"),
    "lm2d_small": lambda: landmark2d_problem(80, 200, 32),
    "lm2d_interleaved": lambda: landmark2d_problem(60, 150, 33, interleave=True, name="lm2d_interleaved"),
    "slam2d_small": lambda: slam2d_problem(60, 90, 68, name="slam2d_small"),
    "slam2d_interleaved": lambda: slam2d_problem(150, 300, 62, interleave=True, name="slam2d_interleaved"),
    "slam3d_small": lambda: slam3d_problem(40, 60, 71, name="slam3d_small"),
    "slam3d_interleaved": lambda: slam3d_problem(150, 300, 73, interleave=True, name="slam3d_interleaved", hubs=26),
    "lm3d_small": lambda: landmark3d_problem(40, 60, 72),
    "rocv_small": lambda: rocv_problem(40, 5, 81, name="rocv_small"),
    "rocv_interleaved": lambda: rocv_problem(150, 8, 83, interleave=True, n_ranges=6, hub=3, name="rocv_interleaved"),
    "stereo_small": lambda: stereo_problem(6, 40, 16, name="stereo_small"),
    "stereo_interleaved": lambda: stereo_problem(30, 150, 17, interleave=True, hubs=True, name="stereo_interleaved"),
    "sim3_small": lambda: sim3_problem(6, 40, 26, name="sim3_small"),
    "sim3_interleaved": lambda: sim3_problem(30, 150, 27, interleave=True, hubs=True, name="sim3_interleaved"),
    "bai_tiny": lambda: bai_tiny(),
    "bai_small": lambda: bai_small(),
    "bai_hub": lambda: bai_hub(),
    "se2_small": lambda: se2_problem(300, 150, 12, name="se2_small"),
    "se3_small": lambda: se3_problem(8, 12, 13, name="se3_small"),
}


def make(name):
    return CONFIGS[name]()
