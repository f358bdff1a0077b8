"""File formats on either side of the hot path, so that fixtures are interchangeable with
the reference and real datasets can be ingested the moment they are supplied.

* MatrixMarket + block layout pair written by `slam_plus_plus -dsm` (system.mtx / system.bla):
  reference writer src/slam/BlockMatrix.cpp:12063-12205 (Save_BlockLayout, Save_MatrixMarket), reader
  :11589,11682-12060. `.bla` = "rows x cols (nnz)" / "brows x bcols (nblocks)" / row bases + total /
  column bases + total. A symmetric dump lists the stored UPPER triangle as lower-triangle coordinates
  (col+1, row+1, value), values printed with %.15g / %.15f.
* SLAM++ / g2o-style text graphs: the token set of include/slam_app/ParsePrimitives.h:75-1665 that
  the five BASELINE.json configs use (2D poses, 3D poses, BA cameras / points / projections).
  Geometry (Jacobian evaluation) stays with the reference; for 2D pose graphs `se2_linearize`
  provides the analytic Jacobians so that a graph file can be turned into hot-path inputs.
"""
import numpy as np

from .blockcsc import BlockCSC, structure_from_pairs


# --------------------------------------------------------------------------------------------------
# system.mtx / system.bla
# --------------------------------------------------------------------------------------------------
def save_matrix_market(path_mtx, path_bla, lam, kind="lambda"):
    """Write Lambda (upper block triangle) the way CUberBlockMatrix::Save_MatrixMarket(..., 'U') does."""
    di = lam.dim[lam.row_idx].astype(np.int64)
    dj = lam.dim[lam.col_idx].astype(np.int64)
    rows, cols, vals = [], [], []
    for p in range(lam.nnzb):
        i, j = int(lam.row_idx[p]), int(lam.col_idx[p])
        blk = lam.vals[lam.blk_off[p]:lam.blk_off[p] + di[p] * dj[p]].reshape(dj[p], di[p]).T
        r = lam.base[i] + np.arange(di[p])[:, None]
        c = lam.base[j] + np.arange(dj[p])[None, :]
        keep = (c >= r)
        rows.append(np.broadcast_to(r, blk.shape)[keep])
        cols.append(np.broadcast_to(c, blk.shape)[keep])
        vals.append(blk[keep])
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    with open(path_mtx, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real symmetric\n")
        f.write("%-------------------------------------------------------------------------------\n")
        f.write("% UberBlockMatrix matrix dump\n% kind: " + kind + "\n")
        f.write("%-------------------------------------------------------------------------------\n")
        f.write("%d %d %d\n" % (lam.n, lam.n, vals.size))
        for r, c, v in zip(rows, cols, vals):  # lower-triangle coordinates: (col + 1, row + 1)
            f.write(("%d %d %.15f\n" if abs(v) > 1 else "%d %d %.15g\n") % (c + 1, r + 1, v))
    with open(path_bla, "w") as f:
        f.write("%d x %d (%d)\n" % (lam.n, lam.n, int((di * dj).sum())))
        f.write("%d x %d (%d)\n" % (lam.nb, lam.nb, lam.nnzb))
        f.write(" ".join(str(int(b)) for b in lam.base) + "\n")
        f.write(" ".join(str(int(b)) for b in lam.base) + "\n")


def load_block_layout(path_bla):
    with open(path_bla) as f:
        lines = [ln.strip() for ln in f if ln.strip()]
    n = int(lines[0].split()[0])
    nb = int(lines[1].split()[0])
    base = np.array(lines[2].split(), dtype=np.int64)
    assert base.size == nb + 1 and base[-1] == n and base[0] == 0
    return n, nb, base


def load_matrix_market(path_mtx, path_bla):
    """Read a (symmetric or general) MatrixMarket file plus its block layout into an upper BlockCSC.
    Entries below the diagonal of a general file are ignored; every block that holds at least one
    entry is materialized fully (missing entries are zero), diagonal blocks are mirrored."""
    n, nb, base = load_block_layout(path_bla)
    dim = np.diff(base).astype(np.int32)
    rr, cc, vv = [], [], []
    symmetric = False
    with open(path_mtx) as f:
        header = None
        for ln in f:
            if ln.startswith("%%MatrixMarket"):
                symmetric = "symmetric" in ln
                continue
            if ln.startswith("%") or not ln.strip():
                continue
            if header is None:
                header = ln.split()
                assert int(header[0]) == n and int(header[1]) == n
                continue
            a, b, v = ln.split()
            rr.append(int(a) - 1)
            cc.append(int(b) - 1)
            vv.append(float(v))
    rr, cc, vv = np.array(rr, dtype=np.int64), np.array(cc, dtype=np.int64), np.array(vv)
    if symmetric:  # stored as lower-triangle coordinates: flip into the upper triangle
        lo = rr > cc
        rr, cc = np.where(lo, cc, rr), np.where(lo, rr, cc)
    keep = rr <= cc
    rr, cc, vv = rr[keep], cc[keep], vv[keep]
    brow = np.searchsorted(base, rr, side="right") - 1
    bcol = np.searchsorted(base, cc, side="right") - 1
    st, blk, _ = structure_from_pairs(dim, brow, bcol)
    vals = np.zeros(st.nvals)
    di = dim[brow].astype(np.int64)
    pos = st.blk_off[blk] + (rr - base[brow]) + (cc - base[bcol]) * di
    vals[pos] = vv
    # mirror the diagonal blocks (the reference stores them fully symmetric)
    dsel = brow == bcol
    pos_t = st.blk_off[blk[dsel]] + (cc[dsel] - base[bcol[dsel]]) + (rr[dsel] - base[brow[dsel]]) * di[dsel]
    vals[pos_t] = vv[dsel]
    return st.with_vals(vals)


# --------------------------------------------------------------------------------------------------
# text graphs
# --------------------------------------------------------------------------------------------------
_SE2_EDGE = {"EDGE_SE2", "EDGE2", "EDGE", "ODOMETRY"}
_SE2_VERTEX = {"VERTEX_SE2", "VERTEX2", "VERTEX"}
_SE3_EDGE = {"EDGE3", "EDGE_SE3", "EDGE3:AXISANGLE", "EDGE_SE3:AXISANGLE"}
_SE3_VERTEX = {"VERTEX3", "VERTEX_SE3"}


def _upper_to_full(u, d):
    m = np.zeros((d, d))
    m[np.triu_indices(d)] = u
    return m + np.triu(m, 1).T


def load_graph(path):
    """Parse the tokens the BASELINE configs use. Returns a dict of numpy arrays:
      se2_vertices (id, x, y, theta), se2_edges (i, j, dx, dy, dtheta) + se2_info (3x3 each)
      se3_vertices (id, 6: t + roll pitch yaw as in the file), se3_edges (i, j, t, AXIS-ANGLE: the parser's conversion
      of roll-pitch-yaw is applied to EDGE3 / EDGE_SE3, EDGE3:AXISANGLE is taken as it stands) + se3_info (6x6 each)
      cams (id, 6 pose + 5 intrinsics), points (id, xyz), projections (point id, cam id, u, v) + proj_info (2x2)
    2D information is given as the 6 upper-triangular values in the order of
    ParsePrimitives.h (xx xy yy tt xt yt for the classic EDGE2 format is NOT assumed: the g2o
    EDGE_SE2 order xx xy xt yy yt tt is)."""
    out = {k: [] for k in ("se2_vertices", "se2_edges", "se2_info", "se3_vertices", "se3_edges", "se3_info",
                           "cams", "points", "projections", "proj_info")}
    with open(path) as f:
        for ln in f:
            t = ln.split()
            if not t or t[0].startswith("#") or t[0].startswith("%"):
                continue
            tok, a = t[0].upper(), t[1:]
            if tok in _SE2_VERTEX and len(a) >= 4:
                out["se2_vertices"].append([float(x) for x in a[:4]])
            elif tok in _SE2_EDGE and len(a) >= 11:
                out["se2_edges"].append([float(x) for x in a[:5]])
                out["se2_info"].append(_upper_to_full([float(x) for x in a[5:11]], 3))
            elif tok in _SE3_VERTEX and len(a) >= 7:
                out["se3_vertices"].append([float(x) for x in a[:7]])
            elif tok in _SE3_EDGE and len(a) >= 29:
                m = [float(x) for x in a[:8]]
                if not tok.endswith(":AXISANGLE"):
                    # roll-pitch-yaw -> axis-angle exactly as the parser does (ParsePrimitives.h:504-519): Q = Rz Ry Rx
                    from scipy.spatial.transform import Rotation
                    m[5:8] = Rotation.from_euler("ZYX", [m[7], m[6], m[5]]).as_rotvec().tolist()
                out["se3_edges"].append(m)
                out["se3_info"].append(_upper_to_full([float(x) for x in a[8:29]], 6))
            elif tok == "VERTEX_CAM" and len(a) >= 13:
                out["cams"].append([float(x) for x in a[:13]])
            elif tok == "VERTEX_XYZ" and len(a) >= 4:
                out["points"].append([float(x) for x in a[:4]])
            elif tok in ("EDGE_PROJECT_P2MC", "EDGE_PROJECT_P2C") and len(a) >= 7:
                out["projections"].append([float(x) for x in a[:4]])
                out["proj_info"].append(_upper_to_full([float(x) for x in a[4:7]], 2))
            # CONSISTENCY_MARKER and unknown tokens are skipped (batch mode ignores them)
    return {k: np.array(v) for k, v in out.items()}


def save_se2_graph(path, poses, edges, info):
    """poses: (n, 3) x y theta; edges: (m, 5) i j dx dy dtheta; info: (m, 3, 3)"""
    with open(path, "w") as f:
        for i, p in enumerate(poses):
            f.write("VERTEX_SE2 %d %.17g %.17g %.17g\n" % (i, p[0], p[1], p[2]))
        iu = np.triu_indices(3)
        for e, m in zip(edges, info):
            f.write("EDGE_SE2 %d %d %.17g %.17g %.17g " % (int(e[0]), int(e[1]), e[2], e[3], e[4]))
            f.write(" ".join("%.17g" % x for x in m[iu]) + "\n")


def save_se3_graph(path, edges, info, poses=None):
    """3D pose graph in the reference's text format. edges: (m, 8) i j tx ty tz ax ay az (relative pose,
    rotation as axis-angle) written as `EDGE3:AXISANGLE` (ParsePrimitives.h:556-617: the measurement is taken
    as it stands, no roll-pitch-yaw conversion), info: (m, 6, 6) -> its 21 upper-triangular values row by row.
    poses (n, 6) [t | roll pitch yaw] are optional `VERTEX3` lines (:741-797, RPY as the parser expects);
    without them the reference initializes every pose by composing the edges, as it does for sphere2500."""
    iu = np.triu_indices(6)
    with open(path, "w") as f:
        if poses is not None:
            for i, p in enumerate(poses):
                f.write("VERTEX3 %d " % i + " ".join("%.17g" % x for x in p) + "\n")
        for e, m in zip(edges, info):
            f.write("EDGE3:AXISANGLE %d %d " % (int(e[0]), int(e[1])) + " ".join("%.17g" % x for x in e[2:8]) + " ")
            f.write(" ".join("%.17g" % x for x in np.asarray(m)[iu]) + "\n")


def save_ba_graph(path, cams, intr, points, obs, info=None, cam_id=None, pt_id=None):
    """Bundle adjustment graph in the reference's text format (data/Readme.txt, ParsePrimitives.h:861-931,
    805-850, 1123-1184): `VERTEX_CAM id x y z qx qy qz qw fx fy cx cy d` stores the camera-to-world pose (centre
    + quaternion), which the parser inverts into the world-to-camera [R | t] it optimizes; `VERTEX_XYZ id x y z`;
    `EDGE_PROJECT_P2MC point-id cam-id u v xx xy yy`.
      cams (nc, 6) world-to-camera [t | axis-angle] (the reference's internal CVertexCam state), intr (nc, 5)
      fx fy cx cy d, points (np, 3), obs (no, 4) point index, camera index, u, v; info (no, 2, 2) or None (identity);
      cam_id / pt_id: vertex ids (default: cameras 0..nc-1, points nc..nc+np-1)."""
    from scipy.spatial.transform import Rotation
    cams, intr, points, obs = (np.asarray(a, dtype=np.float64) for a in (cams, intr, points, obs))
    nc, npts = cams.shape[0], points.shape[0]
    cam_id = np.arange(nc) if cam_id is None else np.asarray(cam_id)
    pt_id = nc + np.arange(npts) if pt_id is None else np.asarray(pt_id)
    R = Rotation.from_rotvec(cams[:, 3:6])
    C = -R.inv().apply(cams[:, :3])            # camera centre in the world
    q = R.inv().as_quat()                       # x y z w, camera-to-world
    order = np.argsort(np.concatenate([cam_id, pt_id]), kind="stable")
    with open(path, "w") as f:
        for v in order:                         # vertices in id order, as the incremental datasets have them
            if v < nc:
                f.write("VERTEX_CAM %d " % cam_id[v] + " ".join("%.17g" % x for x in (*C[v], *q[v], *intr[v])) + "\n")
            else:
                f.write("VERTEX_XYZ %d " % pt_id[v - nc] + " ".join("%.17g" % x for x in points[v - nc]) + "\n")
        for k, o in enumerate(obs):
            m = np.eye(2) if info is None else np.asarray(info[k])
            f.write("EDGE_PROJECT_P2MC %d %d %.17g %.17g %.17g %.17g %.17g\n" % (
                pt_id[int(o[0])], cam_id[int(o[1])], o[2], o[3], m[0, 0], m[0, 1], m[1, 1]))


def load_bal(path):
    """Bundle Adjustment in the Large problem file: `ncams npoints nobs`, nobs lines `cam point x y`, then 9
    numbers per camera (Rodrigues vector, translation, f, k1, k2) and 3 per point. Returns dict(cam_index,
    point_index, xy (nobs, 2), cameras (ncams, 9), points (npoints, 3))."""
    with open(path) as f:
        tok = f.read().split()
    nc, npts, no = int(tok[0]), int(tok[1]), int(tok[2])
    o = np.array(tok[3:3 + 4 * no], dtype=np.float64).reshape(no, 4)
    rest = np.array(tok[3 + 4 * no:3 + 4 * no + 9 * nc + 3 * npts], dtype=np.float64)
    if rest.size != 9 * nc + 3 * npts:
        raise ValueError("truncated BAL file: %s" % path)
    return dict(cam_index=o[:, 0].astype(np.int64), point_index=o[:, 1].astype(np.int64), xy=o[:, 2:4].copy(),
                cameras=rest[:9 * nc].reshape(nc, 9), points=rest[9 * nc:].reshape(npts, 3))


def bal_to_slampp(bal):
    """BAL camera (9 parameters) -> the reference's 6 + 5. BAL projects p = -P / P.z with
    P = R X + t, then f (1 + k1 |p|^2 + k2 |p|^4) p: the camera looks down -z. The reference
    (BASolverBase.h:256-330) projects u = fx x / z + cx with x = R' X + t', then c + (1 + r^2 k) (u - c), r in
    PIXELS and k = d / ((fx + fy) / 2). With F = diag(1, -1, -1): R' = F R, t' = F t, observations (x, -y),
    fx = fy = f, cx = cy = 0; r = f |p| gives k = k1 / f^2, i.e. d = k1 / f. k2 has no counterpart and is dropped.
    The reference's own converter is not in its tree (data/Readme.txt points to an external script), so this
    mapping is derived from the two published camera models and checked by reprojection (tests/test_formats.py).
    Returns (cams (nc, 6) [t' | axis-angle of R'], intr (nc, 5), points, obs (no, 4) point, camera, u, v)."""
    from scipy.spatial.transform import Rotation
    cam = bal["cameras"]
    F = np.diag([1.0, -1.0, -1.0])
    R = Rotation.from_rotvec(cam[:, :3]).as_matrix()
    Rp = np.einsum("ij,cjk->cik", F, R)
    cams = np.concatenate([cam[:, 3:6] @ F.T, Rotation.from_matrix(Rp).as_rotvec()], axis=1)
    f = cam[:, 6]
    intr = np.stack([f, f, np.zeros_like(f), np.zeros_like(f), cam[:, 7] / f], axis=1)
    obs = np.stack([bal["point_index"].astype(np.float64), bal["cam_index"].astype(np.float64),
                    bal["xy"][:, 0], -bal["xy"][:, 1]], axis=1)
    return cams, intr, bal["points"].copy(), obs


def convert_bal_file(path_bal, path_graph):
    """BAL problem file -> VERTEX_CAM / VERTEX_XYZ / EDGE_PROJECT_P2MC graph the reference's parser reads."""
    cams, intr, points, obs = bal_to_slampp(load_bal(path_bal))
    save_ba_graph(path_graph, cams, intr, points, obs)


def se2_linearize(poses, edges, info):
    """Hot-path inputs (synth.Problem) of a 2D pose graph at the given estimate: analytic Jacobians of
    the relative-pose error (the quantity reference include/slam/2DSolverBase.h:269-373 computes),
    residual = measurement - prediction with the angle wrapped to (-pi, pi]."""
    from .synth import Problem
    poses = np.asarray(poses, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    v0 = edges[:, 0].astype(np.int64)
    v1 = edges[:, 1].astype(np.int64)
    ne = v0.size
    c, s = np.cos(poses[v0, 2]), np.sin(poses[v0, 2])
    d = poses[v1, :2] - poses[v0, :2]
    J0 = np.zeros((ne, 3, 3))
    J1 = np.zeros((ne, 3, 3))
    J0[:, 0, 0], J0[:, 0, 1], J0[:, 0, 2] = -c, -s, -s * d[:, 0] + c * d[:, 1]
    J0[:, 1, 0], J0[:, 1, 1], J0[:, 1, 2] = s, -c, -c * d[:, 0] - s * d[:, 1]
    J0[:, 2, 2] = -1
    J1[:, 0, 0], J1[:, 0, 1] = c, s
    J1[:, 1, 0], J1[:, 1, 1] = -s, c
    J1[:, 2, 2] = 1
    pred = np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1], poses[v1, 2] - poses[v0, 2]], axis=1)
    r = edges[:, 2:5] - pred
    r[:, 2] = (r[:, 2] + np.pi) % (2 * np.pi) - np.pi
    return Problem(name="se2_graph", dim=np.full(poses.shape[0], 3, dtype=np.int32), v0=v0, v1=v1, d0=3, d1=3, rd=3,
                   J0=np.ascontiguousarray(J0.transpose(0, 2, 1)).reshape(ne, 9),
                   J1=np.ascontiguousarray(J1.transpose(0, 2, 1)).reshape(ne, 9),
                   Om=np.asarray(info, dtype=np.float64).reshape(ne, 9), r=r, unary_vertex=0, damping=0.0)


def _hat(v):
    z = np.zeros(v.shape[0])
    return np.stack([np.stack([z, -v[:, 2], v[:, 1]], 1), np.stack([v[:, 2], z, -v[:, 0]], 1),
                     np.stack([-v[:, 1], v[:, 0], z], 1)], 1)


def se3_linearize(poses, edges, info):
    """Hot-path inputs (synth.Problem) of a 3D pose graph at the given estimate. poses (n, 6) [t | axis-angle],
    edges (m, 8) i j + 6D measurement, info (m, 6, 6). Expectation C3DJacobians::Absolute_to_Relative, error
    of CEdgePose3D (include/slam/SE3_Types.h:264-286); Jacobians analytic w.r.t. the increments of
    Relative_to_Absolute (the reference takes forward differences there, 3DSolverBase.h:1331-1371)."""
    from scipy.spatial.transform import Rotation
    from .synth import Problem
    poses = np.asarray(poses, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    v0, v1 = edges[:, 0].astype(np.int64), edges[:, 1].astype(np.int64)
    ne = v0.size
    R1 = Rotation.from_rotvec(poses[v0, 3:]).as_matrix()
    R2 = Rotation.from_rotvec(poses[v1, 3:]).as_matrix()
    et = np.einsum("eji,ej->ei", R1, poses[v1, :3] - poses[v0, :3])
    Re = np.einsum("eji,ejk->eik", R1, R2)
    er = Rotation.from_matrix(Re).as_rotvec()
    th = np.linalg.norm(er, axis=1)
    small = th < 1e-4
    ths = np.where(small, 1.0, th)
    c = np.where(small, 1.0 / 12 + th ** 2 / 720, 1 / ths ** 2 - (1 + np.cos(ths)) / (2 * ths * np.sin(ths)))
    K = _hat(er)
    Ji = np.eye(3)[None] + 0.5 * K + c[:, None, None] * np.einsum("eij,ejk->eik", K, K)
    J0 = np.zeros((ne, 6, 6))
    J1 = np.zeros((ne, 6, 6))
    J0[:, :3, :3] = -np.eye(3)
    J0[:, :3, 3:] = _hat(et)
    J0[:, 3:, 3:] = -np.einsum("eij,ekj->eik", Ji, Re)
    J1[:, :3, :3] = Re
    J1[:, 3:, 3:] = Ji
    z = edges[:, 2:8]
    rrot = (Rotation.from_rotvec(z[:, 3:]) * Rotation.from_matrix(Re).inv()).as_rotvec()
    r = np.concatenate([z[:, :3] - et, rrot], axis=1)
    return Problem(name="se3_graph", dim=np.full(poses.shape[0], 6, dtype=np.int32), v0=v0, v1=v1, d0=6, d1=6, rd=6,
                   J0=np.ascontiguousarray(J0.transpose(0, 2, 1)).reshape(ne, 36),
                   J1=np.ascontiguousarray(J1.transpose(0, 2, 1)).reshape(ne, 36),
                   Om=np.asarray(info, dtype=np.float64).reshape(ne, 36), r=r, unary_vertex=0, damping=0.0)


def se3_plus(poses, dx):
    """x (+) dx of CVertexPose3D (C3DJacobians::Relative_to_Absolute): t + R dt, R exp(dr)"""
    from scipy.spatial.transform import Rotation
    R = Rotation.from_rotvec(poses[:, 3:])
    out = np.empty_like(poses)
    out[:, :3] = poses[:, :3] + R.apply(dx[:, :3])
    out[:, 3:] = (R * Rotation.from_rotvec(dx[:, 3:])).as_rotvec()
    return out


def ba_linearize(cams, intr, points, obs, cam_id=None, pt_id=None):
    """Hot-path inputs (synth.Problem) of a bundle adjustment at the given estimate, reference parameterization:
    cams (nc, 6) [t | axis-angle] world -> camera, intr (nc, 5) fx fy cx cy k, points (np, 3), obs (no, 4)
    cam pt u v. Model and increments of CBAJacobians::Project_P2C (include/slam/BASolverBase.h:260-325,559-620;
    analytic where the reference takes forward differences). Vertex ids: cameras 0..nc-1, points nc.. unless
    cam_id / pt_id say otherwise."""
    from scipy.spatial.transform import Rotation
    from .synth import Problem
    cams, intr, points, obs = (np.asarray(a, dtype=np.float64) for a in (cams, intr, points, obs))
    nc, npts, no = cams.shape[0], points.shape[0], obs.shape[0]
    co, po = obs[:, 0].astype(np.int64), obs[:, 1].astype(np.int64)
    cam_id = np.arange(nc) if cam_id is None else np.asarray(cam_id)
    pt_id = nc + np.arange(npts) if pt_id is None else np.asarray(pt_id)
    R = Rotation.from_rotvec(cams[:, 3:]).as_matrix()[co]
    X = points[po]
    x = np.einsum("eij,ej->ei", R, X) + cams[co, :3]
    fx, fy, cx, cy = (intr[co, i] for i in range(4))
    k = intr[co, 4] / (0.5 * (fx + fy))
    iz = 1.0 / x[:, 2]
    d = np.stack([fx * x[:, 0] * iz, fy * x[:, 1] * iz], axis=1)
    r2 = (d ** 2).sum(axis=1)
    g = 1 + r2 * k
    uv = np.stack([cx, cy], axis=1) + g[:, None] * d
    Jd = np.zeros((no, 2, 3))
    Jd[:, 0, 0], Jd[:, 0, 2] = fx * iz, -fx * x[:, 0] * iz * iz
    Jd[:, 1, 1], Jd[:, 1, 2] = fy * iz, -fy * x[:, 1] * iz * iz
    D = g[:, None, None] * np.eye(2)[None] + 2 * k[:, None, None] * np.einsum("ei,ej->eij", d, d)
    PR = np.einsum("eij,ejk,ekl->eil", D, Jd, R)
    J0 = np.concatenate([PR, -np.einsum("eij,ejk->eik", PR, _hat(X))], axis=2)
    dim = np.empty(nc + npts, dtype=np.int32)
    dim[cam_id] = 6
    dim[pt_id] = 3
    return Problem(name="ba", dim=dim, v0=cam_id[co], v1=pt_id[po], d0=6, d1=3, rd=2,
                   J0=np.ascontiguousarray(J0.transpose(0, 2, 1)).reshape(no, 12),
                   J1=np.ascontiguousarray(PR.transpose(0, 2, 1)).reshape(no, 6),
                   Om=np.tile(np.eye(2).ravel(), (no, 1)), r=obs[:, 2:4] - uv, unary_vertex=0, damping=0.0)


def problem_from_graph(path):
    """Graph file -> hot-path inputs (synth.Problem) at the file's initial estimate, plus a short description.
    2D / 3D pose graphs without VERTEX lines are initialized the way the reference's parse loop does it
    (CEdgePose2D / CEdgePose3D constructors: an unseen second vertex becomes first (+) measurement, in file order);
    BA files use the reference's VERTEX_CAM convention (camera-to-world in the file); a file with EDGE_PROJECT_P2SC /
    EDGE_P2SC lines goes to load_stereo_graph and comes back as one (6, 3, 3) group (stereo_linearize). A file with
    LANDMARK3:XYZ / EDGE_SE3_XYZ lines goes to load_slam3d_graph and comes back as the PAIR of its edge groups
    (slam3d_linearize); a file with ROCV: lines goes to load_rocv_graph and comes back as its THREE groups (rocv_linearize);
    a file with VERTEX_CAM:SIM3 lines goes to load_sim3_graph and comes back as one (7, 3, 2) group (sim3_ba_linearize)."""
    from scipy.spatial.transform import Rotation
    with open(path) as f:
        toks = {ln.split()[0].upper() for ln in f if ln.split()}
    has_lm3 = bool(toks & _LM3_XYZ_EDGE)
    if _SIM3_CAM_TOKEN in toks:  # Sim(3) BA, told by its camera token (the edge token is the mono BA's): ONE (7, 3, 2) group
        g = load_sim3_graph(path)
        prob = sim3_ba_linearize(g["cams"], g["intr"], g["points"], g["obs"], g["cam_id"], g["pt_id"], g["info"])
        prob["nc"], prob["npts"] = g["cam_id"].size, g["pt_id"].size
        return prob, "Sim(3) BA graph file (%d cameras, %d points, %d observations)" % (
            g["cam_id"].size, g["pt_id"].size, g["obs"].shape[0])
    if toks & _ROCV_TOKENS:  # range-only constant velocity: THREE edge groups, the last one unary (nonlinear.CRocv)
        s = load_rocv_graph(path)
        groups = rocv_linearize(s["dim"], s["state"], s["cv"], s["cv_info"], s["rng"], s["rng_info"], s["pri"], s["pri_info"])
        return groups, "ROCV graph file (%d receivers, %d transmitters, %d constant-velocity edges, %d ranges, %d priors)" % (
            int((s["dim"] == 6).sum()), int((s["dim"] == 3).sum()), s["cv"].shape[0], s["rng"].shape[0], s["pri"].size)
    if toks & _P2SC_EDGE:  # stereo BA: ONE (6, 3, 3) group, cameras CVertexSCam
        g = load_stereo_graph(path)
        prob = stereo_linearize(g["cams"], g["intr"], g["points"], g["obs"], g["cam_id"], g["pt_id"], g["info"])
        prob["nc"], prob["npts"] = g["cam_id"].size, g["pt_id"].size
        return prob, "stereo BA graph file (%d cameras, %d points, %d observations)" % (
            g["cam_id"].size, g["pt_id"].size, g["obs"].shape[0])
    if has_lm3:  # 3D poses + landmarks: TWO edge groups over the same vertices (nonlinear.CSlam3D solves such a graph)
        s = load_slam3d_graph(path)
        groups = slam3d_linearize(s["dim"], s["state"], s["odo"], s["odo_info"], s["obs"], s["obs_info"])
        return groups, "3D landmark SLAM graph file (%d poses, %d landmarks, %d odometry edges, %d observations)" % (
            int((s["dim"] == 6).sum()), int((s["dim"] == 3).sum()), s["odo"].shape[0], s["obs"].shape[0])
    g = load_graph(path)
    if g["projections"].size:
        cams_f, pts_f, proj = g["cams"], g["points"], g["projections"]
        q = Rotation.from_quat(cams_f[:, 4:8]).inv()          # the parser's inversion (ParsePrimitives.h:886-905)
        cams = np.concatenate([q.apply(-cams_f[:, 1:4]), q.as_rotvec()], axis=1)
        ids = np.concatenate([cams_f[:, 0], pts_f[:, 0]]).astype(np.int64)
        nv = int(ids.max()) + 1
        cam_id, pt_id = cams_f[:, 0].astype(np.int64), pts_f[:, 0].astype(np.int64)
        cam_index = np.full(nv, -1, dtype=np.int64)
        cam_index[cam_id] = np.arange(cam_id.size)
        pt_index = np.full(nv, -1, dtype=np.int64)
        pt_index[pt_id] = np.arange(pt_id.size)
        obs = np.stack([cam_index[proj[:, 1].astype(np.int64)].astype(np.float64),     # ba_linearize: cam pt u v
                        pt_index[proj[:, 0].astype(np.int64)].astype(np.float64), proj[:, 2], proj[:, 3]], axis=1)
        prob = ba_linearize(cams, cams_f[:, 8:13], pts_f[:, 1:4], obs, cam_id=cam_id, pt_id=pt_id)
        prob["Om"] = np.ascontiguousarray(g["proj_info"]).reshape(-1, 4)
        prob["nc"], prob["npts"] = cam_id.size, pt_id.size
        return prob, "BA graph file (%d cameras, %d points, %d observations)" % (cam_id.size, pt_id.size, obs.shape[0])
    if g["se3_edges"].size:
        e = g["se3_edges"]
        n = int(e[:, :2].max()) + 1
        poses = np.zeros((n, 6))
        seen = np.zeros(n, dtype=bool)
        for v in g["se3_vertices"].reshape(-1, 7):  # VERTEX3: t + roll pitch yaw (ParsePrimitives.h:741-797)
            poses[int(v[0])] = np.concatenate([v[1:4], Rotation.from_euler("ZYX", [v[6], v[5], v[4]]).as_rotvec()])
            seen[int(v[0])] = True
        if not seen.any():
            seen[int(e[0, 0])] = True
        for a, b, *z in e:
            a, b = int(a), int(b)
            if seen[a] and not seen[b]:
                poses[b] = se3_plus(poses[a:a + 1], np.asarray(z)[None, :])[0]
                seen[b] = True
        if not seen.all():
            raise ValueError("3D pose graph: %d poses are not reachable through forward edges" % int((~seen).sum()))
        return se3_linearize(poses, e, g["se3_info"]), "3D pose graph file (%d poses, %d edges)" % (n, e.shape[0])
    if g["se2_edges"].size:
        e = g["se2_edges"]
        n = int(e[:, :2].max()) + 1
        poses = np.zeros((n, 3))
        seen = np.zeros(n, dtype=bool)
        for v in g["se2_vertices"].reshape(-1, 4):
            poses[int(v[0])] = v[1:4]
            seen[int(v[0])] = True
        if not seen.any():
            seen[int(e[0, 0])] = True
        for a, b, dx, dy, dt in e:
            a, b = int(a), int(b)
            if seen[a] and not seen[b]:
                c, s = np.cos(poses[a, 2]), np.sin(poses[a, 2])
                poses[b] = [poses[a, 0] + c * dx - s * dy, poses[a, 1] + s * dx + c * dy, poses[a, 2] + dt]
                seen[b] = True
        if not seen.all():
            raise ValueError("2D pose graph: %d poses are not reachable through forward edges" % int((~seen).sum()))
        return se2_linearize(poses, e, g["se2_info"]), "2D pose graph file (%d poses, %d edges)" % (n, e.shape[0])
    raise ValueError("no edges of a known type in %s" % path)


# --------------------------------------------------------------------------------------------------
# 2D landmark SLAM: poses (3) + point landmarks (2), odometry + range-bearing observations
# --------------------------------------------------------------------------------------------------
_LM2_XY_EDGE = {"LANDMARK2:XY", "EDGE_SE2_XY", "EDGE_BEARING_SE2_XY", "LANDMARK"}   # ParsePrimitives.h:270-273
_LM2_RB_EDGE = {"LANDMARK2:RB", "EDGE_SE2_RB", "EDGE_BEARING_SE2_RB"}                # :363-365
_TWO_PI = 2 * np.pi


def _clamp_angle_2pi(a):
    """C2DJacobians::f_ClampAngle_2Pi (2DSolverBase.h:44-67)"""
    return np.fmod(a, _TWO_PI)


def _clamp_angular_error_2pi(e):
    """C2DJacobians::f_ClampAngularError_2Pi (2DSolverBase.h:79-94): the smallest in magnitude of e, e - 2 pi, e + 2 pi"""
    e = np.fmod(e, _TWO_PI)
    a, b = e - _TWO_PI, e + _TWO_PI
    m = np.where(np.abs(e) < np.abs(a), e, a)
    return np.where(np.abs(m) < np.abs(b), m, b)


def _se2_compose(p, d):
    """C2DJacobians::Relative_to_Absolute (2DSolverBase.h:96-130): p (+) d, angle clamped"""
    c, s = np.cos(p[2]), np.sin(p[2])
    return np.array([p[0] + c * d[0] - s * d[1], p[1] + s * d[0] + c * d[1], _clamp_angle_2pi(p[2] + d[2])])


def slam2d_offsets(dim):
    base = np.zeros(len(dim) + 1, dtype=np.int64)
    np.cumsum(dim, out=base[1:])
    return base


def load_slam2d_graph(path):
    """A 2D landmark SLAM graph as the reference's parser and edge constructors would build it, line by line. Returns
      dim (nv,) 3 for a pose / 2 for a landmark, state (flat, laid out by dim), vertex ids 0 .. nv - 1,
      odo (m, 5) i j dx dy dtheta + odo_info (m, 3, 3) + odo_seq (m,) position among all edges of the file,
      obs (k, 4) pose landmark range bearing + obs_info (k, 2, 2) + obs_seq (k,).
    Tokens: VERTEX_SE2 / VERTEX2 / VERTEX (ParsePrimitives.h:420-422; the parser has NO token for a 2D landmark vertex),
    the odometry tokens of load_graph, the XY landmark tokens (:270-273) and the RB ones (:363-365).
    * an XY measurement is converted to polar and its information REPLACED BY THE IDENTITY (CEdgePoseLandmark2D::v_ToPolar /
      t_ToPolar, SE2_Types.h:602-616; the parser itself warns that chi2 is then incorrect); RB tokens keep both;
    * an edge that names the landmark first is swapped (SE2_Types.h:437-442: a known first vertex of width 2, or a known
      second one of width 3), so obs[:, 0] is always the pose;
    * a vertex an edge meets first is initialised from it: a pose by composing the odometry (the null vertex for the
      very first), a landmark by CRelative_to_Absolute_XY_Initializer (pose (+) (dx, dy), SE2_Types.h:381-409) or by
      CRelative_to_Absolute_RangeBearing_Initializer (:347-375). The latter is mirrored as written: it composes the pose
      with (range, 0, bearing) and stores (the NORM of the resulting position, the resulting angle) as the landmark."""
    state, dimof = {}, {}
    odo, odo_info, odo_seq, obs, obs_info, obs_seq = [], [], [], [], [], []
    n_edges = 0

    def known(v, d):
        return v in state and dimof[v] == d

    with open(path) as f:
        for ln in f:
            t = ln.split()
            if not t or t[0].startswith("#") or t[0].startswith("%"):
                continue
            tok, a = t[0].upper(), t[1:]
            if tok in _SE2_VERTEX and len(a) >= 4:
                v = int(a[0])
                state[v], dimof[v] = np.array([float(x) for x in a[1:4]]), 3
            elif tok in _SE2_EDGE and len(a) >= 11:
                i, j = int(a[0]), int(a[1])
                z = np.array([float(x) for x in a[2:5]])
                if i not in state:
                    state[i], dimof[i] = np.zeros(3), 3           # CInitializeNullVertex
                if j not in state:
                    state[j], dimof[j] = _se2_compose(state[i], z), 3
                odo.append([i, j, *z])
                odo_info.append(_upper_to_full([float(x) for x in a[5:11]], 3))
                odo_seq.append(n_edges)
                n_edges += 1
            elif (tok in _LM2_XY_EDGE or tok in _LM2_RB_EDGE) and len(a) >= 7:
                i, j = int(a[0]), int(a[1])
                z = np.array([float(a[2]), float(a[3])])
                info = _upper_to_full([float(x) for x in a[4:7]], 2)
                if known(i, 2) or known(j, 3):
                    i, j = j, i
                if i not in state:
                    state[i], dimof[i] = np.zeros(3), 3
                if tok in _LM2_XY_EDGE:
                    if j not in state:
                        state[j], dimof[j] = _se2_compose(state[i], [z[0], z[1], 0.0])[:2], 2
                    z = np.array([np.hypot(z[0], z[1]), _clamp_angle_2pi(np.arctan2(z[1], z[0]))])
                    info = np.eye(2)
                elif j not in state:
                    q = _se2_compose(state[i], [z[0], 0.0, z[1]])
                    state[j], dimof[j] = np.array([np.hypot(q[0], q[1]), q[2]]), 2
                obs.append([i, j, *z])
                obs_info.append(info)
                obs_seq.append(n_edges)
                n_edges += 1
    nv = max(state) + 1 if state else 0
    if sorted(state) != list(range(nv)):
        raise ValueError("vertex ids are not 0 .. n-1: %s" % path)
    dim = np.array([dimof[v] for v in range(nv)], dtype=np.int32)
    return dict(dim=dim, state=np.concatenate([state[v] for v in range(nv)]) if nv else np.zeros(0),
                odo=np.array(odo).reshape(-1, 5), odo_info=np.array(odo_info).reshape(-1, 3, 3),
                odo_seq=np.array(odo_seq, dtype=np.int64), obs=np.array(obs).reshape(-1, 4),
                obs_info=np.array(obs_info).reshape(-1, 2, 2), obs_seq=np.array(obs_seq, dtype=np.int64))


def save_slam2d_graph(path, dim, state, odo, odo_info, obs, obs_info, odo_seq=None, obs_seq=None):
    """VERTEX_SE2 for every pose (landmarks have no vertex token: the reader initialises them from their first
    observation), EDGE_SE2 and EDGE_SE2_RB (range bearing + the 3 upper values of the information) in the global edge
    order, everything with %.17g."""
    dim = np.asarray(dim)
    base = slam2d_offsets(dim)
    m, k = len(odo), len(obs)
    odo_seq = np.arange(m) if odo_seq is None else np.asarray(odo_seq)
    obs_seq = m + np.arange(k) if obs_seq is None else np.asarray(obs_seq)
    lines = [None] * (m + k)
    iu = np.triu_indices(3)
    for e, mat, q in zip(odo, odo_info, odo_seq):
        lines[q] = "EDGE_SE2 %d %d %.17g %.17g %.17g " % (int(e[0]), int(e[1]), e[2], e[3], e[4]) + \
            " ".join("%.17g" % x for x in np.asarray(mat)[iu])
    for e, mat, q in zip(obs, obs_info, obs_seq):
        mat = np.asarray(mat)
        lines[q] = "EDGE_SE2_RB %d %d %.17g %.17g %.17g %.17g %.17g" % (int(e[0]), int(e[1]), e[2], e[3],
                                                                        mat[0, 0], mat[0, 1], mat[1, 1])
    with open(path, "w") as f:
        for v in np.flatnonzero(dim == 3):
            f.write("VERTEX_SE2 %d %.17g %.17g %.17g\n" % (v, *state[base[v]:base[v] + 3]))
        f.write("\n".join(lines) + "\n")


def slam2d_linearize(dim, state, odo, odo_info, obs, obs_info, unary_vertex=0):
    """The two edge groups of a 2D landmark SLAM graph at `state` (flat, laid out by dim), as synth.Problems over the
    SAME vertices: odometry (3, 3, 3) -- C2DJacobians::Absolute_to_Relative, 2DSolverBase.h:373-418, error of CEdgePose2D --
    and observations (3, 2, 2) -- Observation2D_RangeBearing, :443-496 (range floored at 1e-5 before the Jacobians),
    error of CEdgePoseLandmark2D with the bearing wrapped, SE2_Types.h:562-573. Angles are clamped exactly as there."""
    from .synth import Problem
    dim = np.asarray(dim, dtype=np.int32)
    x = np.asarray(state, dtype=np.float64)
    base = slam2d_offsets(dim)
    odo = np.asarray(odo, dtype=np.float64).reshape(-1, 5)
    obs = np.asarray(obs, dtype=np.float64).reshape(-1, 4)
    # odometry
    v0, v1 = odo[:, 0].astype(np.int64), odo[:, 1].astype(np.int64)
    m = v0.size
    p1 = x[base[v0][:, None] + np.arange(3)]
    p2 = x[base[v1][:, None] + np.arange(3)]
    c, s = np.cos(p1[:, 2]), np.sin(p1[:, 2])
    d = p2[:, :2] - p1[:, :2]
    J0, J1 = np.zeros((m, 3, 3)), np.zeros((m, 3, 3))
    J0[:, 0, 0], J0[:, 0, 1], J0[:, 0, 2] = -c, -s, -s * d[:, 0] + c * d[:, 1]
    J0[:, 1, 0], J0[:, 1, 1], J0[:, 1, 2] = s, -c, -c * d[:, 0] - s * d[:, 1]
    J0[:, 2, 2] = -1
    J1[:, 0, 0], J1[:, 0, 1] = c, s
    J1[:, 1, 0], J1[:, 1, 1] = -s, c
    J1[:, 2, 2] = 1
    r = np.empty((m, 3))
    r[:, 0] = odo[:, 2] - (c * d[:, 0] + s * d[:, 1])
    r[:, 1] = odo[:, 3] - (-s * d[:, 0] + c * d[:, 1])
    r[:, 2] = _clamp_angular_error_2pi(odo[:, 4] - _clamp_angle_2pi(p2[:, 2] - p1[:, 2]))
    g_odo = Problem(name="slam2d_odometry", dim=dim, v0=v0, v1=v1, d0=3, d1=3, rd=3,
                    J0=np.ascontiguousarray(J0.transpose(0, 2, 1)).reshape(m, 9),
                    J1=np.ascontiguousarray(J1.transpose(0, 2, 1)).reshape(m, 9),
                    Om=np.asarray(odo_info, dtype=np.float64).reshape(m, 9), r=r, unary_vertex=unary_vertex, damping=0.0)
    # observations
    vp, vl = obs[:, 0].astype(np.int64), obs[:, 1].astype(np.int64)
    k = vp.size
    p = x[base[vp][:, None] + np.arange(3)]
    l = x[base[vl][:, None] + np.arange(2)]
    de, dn = l[:, 0] - p[:, 0], l[:, 1] - p[:, 1]
    rng = np.sqrt(de * de + dn * dn)
    hb = _clamp_angle_2pi(np.arctan2(dn, de) - p[:, 2])
    rng = np.where(np.abs(rng) < 1e-5, 1e-5, rng)
    d2 = rng * rng
    H0, H1 = np.zeros((k, 2, 3)), np.zeros((k, 2, 2))
    H0[:, 0, 0], H0[:, 0, 1] = -de / rng, -dn / rng
    H0[:, 1, 0], H0[:, 1, 1], H0[:, 1, 2] = dn / d2, -de / d2, -1
    H1[:, 0, 0], H1[:, 0, 1] = de / rng, dn / rng
    H1[:, 1, 0], H1[:, 1, 1] = -dn / d2, de / d2
    ro = np.empty((k, 2))
    ro[:, 0] = obs[:, 2] - rng
    ro[:, 1] = _clamp_angular_error_2pi(obs[:, 3] - hb)
    g_obs = Problem(name="slam2d_observations", dim=dim, v0=vp, v1=vl, d0=3, d1=2, rd=2,
                    J0=np.ascontiguousarray(H0.transpose(0, 2, 1)).reshape(k, 6),
                    J1=np.ascontiguousarray(H1.transpose(0, 2, 1)).reshape(k, 4),
                    Om=np.asarray(obs_info, dtype=np.float64).reshape(k, 4), r=ro, unary_vertex=unary_vertex, damping=0.0)
    return g_odo, g_obs


# --------------------------------------------------------------------------------------------------
# 3D landmark SLAM: poses (6, [t | axis-angle]) + point landmarks (3), odometry + XYZ observations
# --------------------------------------------------------------------------------------------------
_LM3_XYZ_EDGE = {"LANDMARK3:XYZ", "EDGE_SE3_XYZ"}   # ParsePrimitives.h:639-640


def slam3d_offsets(dim):
    return slam2d_offsets(dim)


def _rpy_to_rotvec(rpy):
    """the parser's conversion of roll pitch yaw (ParsePrimitives.h:504-519): Q = Rz Ry Rx"""
    from scipy.spatial.transform import Rotation
    return Rotation.from_euler("ZYX", [rpy[2], rpy[1], rpy[0]]).as_rotvec()


def load_slam3d_graph(path):
    """A 3D landmark SLAM graph as the reference's parser and edge constructors would build it, line by line. Returns
      dim (nv,) 6 for a pose / 3 for a landmark, state (flat, laid out by dim), vertex ids 0 .. nv - 1,
      odo (m, 8) i j t (3) axis-angle (3) + odo_info (m, 6, 6) + odo_seq (m,) position among all edges of the file,
      obs (k, 5) pose landmark x y z + obs_info (k, 3, 3) + obs_seq (k,).
    Tokens: the pose edges and VERTEX3 lines of load_graph (roll-pitch-yaw converted unless the token ends in :AXISANGLE)
    and LANDMARK3:XYZ / EDGE_SE3_XYZ: two ids, x y z, the 6 upper-triangular values of the information row by row
    (ParsePrimitives.h:629-680). The first id is the pose (CEdgePoseLandmark3D swaps nothing). A vertex an edge meets
    first is initialised from it: a pose by composing the odometry (the null vertex for the very first), a landmark at
    t + R z of the observing pose (CRelative_to_Absolute_XYZ_Initializer, SE3_Types.h:449-478)."""
    from scipy.spatial.transform import Rotation
    state, dimof = {}, {}
    odo, odo_info, odo_seq, obs, obs_info, obs_seq = [], [], [], [], [], []
    n_edges = 0
    with open(path) as f:
        for ln in f:
            t = ln.split()
            if not t or t[0].startswith("#") or t[0].startswith("%"):
                continue
            tok, a = t[0].upper(), t[1:]
            if tok in _SE3_VERTEX and len(a) >= 7:
                v = [float(x) for x in a[:7]]
                state[int(v[0])], dimof[int(v[0])] = np.concatenate([v[1:4], _rpy_to_rotvec(v[4:7])]), 6
            elif tok in _SE3_EDGE and len(a) >= 29:
                i, j = int(a[0]), int(a[1])
                z = np.array([float(x) for x in a[2:8]])
                if not tok.endswith(":AXISANGLE"):
                    z[3:] = _rpy_to_rotvec(z[3:])
                if i not in state:
                    state[i], dimof[i] = np.zeros(6), 6           # CInitializeNullVertex
                if j not in state:
                    state[j], dimof[j] = se3_plus(state[i][None, :], z[None, :])[0], 6
                odo.append([i, j, *z])
                odo_info.append(_upper_to_full([float(x) for x in a[8:29]], 6))
                odo_seq.append(n_edges)
                n_edges += 1
            elif tok in _LM3_XYZ_EDGE and len(a) >= 11:
                i, j = int(a[0]), int(a[1])
                z = np.array([float(x) for x in a[2:5]])
                if i not in state:
                    state[i], dimof[i] = np.zeros(6), 6
                if j not in state:
                    state[j], dimof[j] = state[i][:3] + Rotation.from_rotvec(state[i][3:]).apply(z), 3
                obs.append([i, j, *z])
                obs_info.append(_upper_to_full([float(x) for x in a[5:11]], 3))
                obs_seq.append(n_edges)
                n_edges += 1
    nv = max(state) + 1 if state else 0
    if sorted(state) != list(range(nv)):
        raise ValueError("vertex ids are not 0 .. n-1: %s" % path)
    for grp, col, d in ((odo, 0, 6), (odo, 1, 6), (obs, 0, 6), (obs, 1, 3)):
        if any(dimof[int(e[col])] != d for e in grp):
            raise ValueError("an edge joins vertices of the wrong widths: %s" % path)
    dim = np.array([dimof[v] for v in range(nv)], dtype=np.int32)
    return dict(dim=dim, state=np.concatenate([state[v] for v in range(nv)]) if nv else np.zeros(0),
                odo=np.array(odo).reshape(-1, 8), odo_info=np.array(odo_info).reshape(-1, 6, 6),
                odo_seq=np.array(odo_seq, dtype=np.int64), obs=np.array(obs).reshape(-1, 5),
                obs_info=np.array(obs_info).reshape(-1, 3, 3), obs_seq=np.array(obs_seq, dtype=np.int64))


def slam3d_lines(odo, odo_info, obs, obs_info, odo_seq=None, obs_seq=None, ids=None):
    """EDGE3:AXISANGLE and EDGE_SE3_XYZ lines in the global edge order, everything with %.17g; ids: vertex id -> id written"""
    m, k = len(odo), len(obs)
    odo_seq = np.arange(m) if odo_seq is None else np.asarray(odo_seq)
    obs_seq = m + np.arange(k) if obs_seq is None else np.asarray(obs_seq)
    name = (lambda v: int(v)) if ids is None else (lambda v: ids[int(v)])
    lines = [None] * (m + k)
    for tok, d, edges, infos, seq in (("EDGE3:AXISANGLE", 6, odo, odo_info, odo_seq), ("EDGE_SE3_XYZ", 3, obs, obs_info, obs_seq)):
        iu = np.triu_indices(d)
        for e, mat, q in zip(edges, infos, seq):
            lines[q] = "%s %d %d " % (tok, name(e[0]), name(e[1])) + " ".join("%.17g" % x for x in e[2:2 + d]) + " " + \
                " ".join("%.17g" % x for x in np.asarray(mat)[iu])
    return lines


def save_slam3d_graph(path, dim, state, odo, odo_info, obs, obs_info, odo_seq=None, obs_seq=None):
    """EDGE3:AXISANGLE and EDGE_SE3_XYZ lines in the global edge order. No vertex lines: VERTEX3 holds roll-pitch-yaw,
    which would not bring an axis-angle back bit for bit, and landmarks have no vertex token here; the reader composes
    the poses from the odometry and puts every landmark where its first observation sees it (dim and state only say
    which graph this is)."""
    with open(path, "w") as f:
        f.write("\n".join(slam3d_lines(odo, odo_info, obs, obs_info, odo_seq, obs_seq)) + "\n")


def slam3d_expectation(pose, lm):
    """C3DJacobians::Absolute_to_Relative_Landmark (3DSolverBase.h:1528-1539): R(a)^T (l - t); pose (k, 6), lm (k, 3)"""
    from scipy.spatial.transform import Rotation
    return Rotation.from_rotvec(pose[:, 3:]).inv().apply(lm - pose[:, :3])


def slam3d_linearize(dim, state, odo, odo_info, obs, obs_info, unary_vertex=0):
    """The two edge groups of a 3D landmark SLAM graph at `state` (flat, laid out by dim), as synth.Problems over the
    SAME vertices: odometry (6, 6, 6) -- se3_linearize above, CEdgePose3D -- and XYZ observations (6, 3, 3):
    expectation e = R(a)^T (l - t), r = z - e without any wrapping (CEdgePoseLandmark3D, SE3_Types.h:568-586), Jacobians
    w.r.t. the pose increment of Relative_to_Absolute (t' = t + R dt, R' = R exp(dr), 3DSolverBase.h:807-850) and w.r.t.
    the landmark: e(t + R dt, R exp(dr)) = exp(dr)^T (e - dt), hence d e / d pose = [-I | [e]x], d e / d l = R^T --
    analytic where the reference takes forward differences with delta = 1e-9 (:1602-1637)."""
    from scipy.spatial.transform import Rotation
    from .synth import Problem
    dim = np.asarray(dim, dtype=np.int32)
    x = np.asarray(state, dtype=np.float64)
    base = slam3d_offsets(dim)
    odo = np.asarray(odo, dtype=np.float64).reshape(-1, 8)
    obs = np.asarray(obs, dtype=np.float64).reshape(-1, 5)
    # odometry: se3_linearize over an array with a row per vertex (landmark rows are never addressed)
    pose_v = np.flatnonzero(dim == 6)
    rows = np.zeros((dim.size, 6))
    rows[pose_v] = x[base[pose_v][:, None] + np.arange(6)]
    g_odo = se3_linearize(rows, odo, np.asarray(odo_info, dtype=np.float64).reshape(-1, 6, 6))
    g_odo["name"], g_odo["dim"], g_odo["unary_vertex"] = "slam3d_odometry", dim, unary_vertex
    # observations
    vp, vl = obs[:, 0].astype(np.int64), obs[:, 1].astype(np.int64)
    k = vp.size
    p = x[base[vp][:, None] + np.arange(6)]
    l = x[base[vl][:, None] + np.arange(3)]
    e = slam3d_expectation(p, l)
    H0 = np.concatenate([np.tile(-np.eye(3), (k, 1, 1)), _hat(e)], axis=2)
    H1 = Rotation.from_rotvec(p[:, 3:]).as_matrix().transpose(0, 2, 1)
    g_obs = Problem(name="slam3d_observations", dim=dim, v0=vp, v1=vl, d0=6, d1=3, rd=3,
                    J0=np.ascontiguousarray(H0.transpose(0, 2, 1)).reshape(k, 18),
                    J1=np.ascontiguousarray(H1.transpose(0, 2, 1)).reshape(k, 9),
                    Om=np.asarray(obs_info, dtype=np.float64).reshape(k, 9), r=obs[:, 2:5] - e, unary_vertex=unary_vertex,
                    damping=0.0)
    return g_odo, g_obs


def slam3d_plus(dim, state, dx):
    """x (+) dx over the flat state: poses by se3_plus (CVertexPose3D::Operator_Plus), landmarks by the plain sum
    (CVertexLandmark3D::Operator_Plus, SE3_Types.h:110-113)"""
    dim = np.asarray(dim)
    base = slam3d_offsets(dim)
    out = state + dx
    idx = base[:-1][dim == 6][:, None] + np.arange(6)
    out[idx] = se3_plus(state[idx], dx[idx])
    return out


# --------------------------------------------------------------------------------------------------
# stereo bundle adjustment: cameras CVertexSCam (6, [t | axis-angle] + 6 intrinsics) + points (3), CEdgeP2SC3D
# --------------------------------------------------------------------------------------------------
_P2SC_EDGE = {"EDGE_PROJECT_P2SC", "EDGE_P2SC"}   # ParsePrimitives.h:1314-1315


def stereo_expectation(cam, intr, X):
    """CBAJacobians::Project_P2SC (include/slam/BASolverBase.h:462-537) as the reference writes it, one row per
    observation: cam (k, 6) [t | axis-angle] world -> left camera, intr (k, 6) fx fy cx cy d b, X (k, 3) -> (k, 3)
    u v u_right. x = R X + t, uv = A x / x2, k = d / (0.5 (fx + fy)), rho = |uv - c|, uv <- c + (1 + rho k)(uv - c); the
    right camera sees the point moved by -b (row 0 of R)^T through the same steps with its own rho."""
    from scipy.spatial.transform import Rotation
    cam, intr, X = (np.asarray(a, dtype=np.float64) for a in (cam, intr, X))
    R = Rotation.from_rotvec(cam[:, 3:6]).as_matrix()
    fx, fy, cx, cy = (intr[:, i] for i in range(4))
    k, b = intr[:, 4] / (0.5 * (fx + fy)), intr[:, 5]
    c = np.stack([cx, cy], axis=1)

    def project(Xw):
        x = np.einsum("eij,ej->ei", R, Xw) + cam[:, :3]
        uv = np.stack([fx * x[:, 0] + cx * x[:, 2], fy * x[:, 1] + cy * x[:, 2]], axis=1) / x[:, 2:3]   # A x / (A x)_2
        rho = np.sqrt(((uv - c) ** 2).sum(axis=1))
        return c + (1 + rho * k)[:, None] * (uv - c)

    uv = project(X)
    uv2 = project(X - b[:, None] * R[:, 0, :])
    return np.stack([uv[:, 0], uv[:, 1], uv2[:, 0]], axis=1)


def stereo_linearize(cams, intr, points, obs, cam_id=None, pt_id=None, info=None):
    """Hot-path inputs (synth.Problem, like ba_linearize: one group, here (6, 3, 3)) of a stereo bundle adjustment at the
    given estimate: cams (nc, 6) [t | axis-angle] world -> left camera, intr (nc, 6) fx fy cx cy d b, points (np, 3), obs
    (no, 5) cam pt u v u_right, info (no, 3, 3) or None (identity). r = z - stereo_expectation. Jacobians w.r.t. the camera
    increment of Relative_to_Absolute (t' = t + R dt, R' = R exp(dr), 3DSolverBase.h:807-850) and the point, analytic
    where the reference takes forward differences with delta = 1e-9 (BASolverBase.h:781-841). With q = p - c,
    rho = |q|: d uv / d q = (1 + rho k) I + k q n^T, n = q / rho and n = 0 at rho = 0 (the term's norm is rho k: it
    vanishes there, a point on the optical axis has finite Jacobians); d q / d x = [fx/x2 0 -fx x0/x2^2; 0 fy/x2
    -fy x1/x2^2]. Since R (row 0 of R)^T = e0 -- for the incremented R' as well -- the right camera's point in the camera
    frame is x - b e0 and has d x / d increment of the left one: P = rows 0, 1 of the left chain, row 0 of the right one
    at x - b e0; J_cam = P [R | -R [X]x], J_pt = P R. Vertex ids: cameras 0..nc-1, points nc.. unless cam_id / pt_id say
    otherwise."""
    from scipy.spatial.transform import Rotation
    from .synth import Problem
    cams, intr, points, obs = (np.asarray(a, dtype=np.float64) for a in (cams, intr, points, obs))
    nc, npts, no = cams.shape[0], points.shape[0], obs.shape[0]
    co, po = obs[:, 0].astype(np.int64), obs[:, 1].astype(np.int64)
    cam_id = np.arange(nc) if cam_id is None else np.asarray(cam_id)
    pt_id = nc + np.arange(npts) if pt_id is None else np.asarray(pt_id)
    R = Rotation.from_rotvec(cams[:, 3:]).as_matrix()[co]
    X = points[po]
    x = np.einsum("eij,ej->ei", R, X) + cams[co, :3]
    fx, fy = intr[co, 0], intr[co, 1]
    k, b = intr[co, 4] / (0.5 * (fx + fy)), intr[co, 5]
    iz = 1.0 / x[:, 2]

    def chain(x0):
        """D Jd (no, 2, 3) of one camera whose point has the first camera-frame coordinate x0"""
        q = np.stack([fx * x0 * iz, fy * x[:, 1] * iz], axis=1)
        rho = np.sqrt((q ** 2).sum(axis=1))
        n = np.where(rho[:, None] > 0, q / np.where(rho > 0, rho, 1.0)[:, None], 0.0)
        D = (1 + rho * k)[:, None, None] * np.eye(2)[None] + k[:, None, None] * np.einsum("ei,ej->eij", q, n)
        Jd = np.zeros((no, 2, 3))
        Jd[:, 0, 0], Jd[:, 0, 2] = fx * iz, -fx * x0 * iz * iz
        Jd[:, 1, 1], Jd[:, 1, 2] = fy * iz, -fy * x[:, 1] * iz * iz
        return np.einsum("eij,ejk->eik", D, Jd)

    P = np.concatenate([chain(x[:, 0]), chain(x[:, 0] - b)[:, :1]], axis=1)
    PR = np.einsum("eij,ejk->eik", P, R)
    J0 = np.concatenate([PR, -np.einsum("eij,ejk->eik", PR, _hat(X))], axis=2)
    dim = np.empty(nc + npts, dtype=np.int32)
    dim[cam_id] = 6
    dim[pt_id] = 3
    Om = np.tile(np.eye(3), (no, 1, 1)) if info is None else np.asarray(info, dtype=np.float64)
    return Problem(name="stereo_ba", dim=dim, v0=cam_id[co], v1=pt_id[po], d0=6, d1=3, rd=3,
                   J0=np.ascontiguousarray(J0.transpose(0, 2, 1)).reshape(no, 18),
                   J1=np.ascontiguousarray(PR.transpose(0, 2, 1)).reshape(no, 9),
                   Om=np.ascontiguousarray(Om).reshape(no, 9), r=obs[:, 2:5] - stereo_expectation(cams[co], intr[co], X),
                   unary_vertex=0, damping=0.0)


def load_stereo_graph(path):
    """A stereo BA graph as the reference's parser reads it: `VERTEX_SCAM id x y z qx qy qz qw fx fy cx cy d b` stores the
    camera-to-world pose (centre + quaternion), which the parser inverts into the world-to-camera [t | axis-angle] it
    optimizes, exactly as for VERTEX_CAM (include/slam_app/ParsePrimitives.h:984-1048: quat.inverse(), c = quat * -t,
    Quat_to_AxisAngle); `VERTEX_XYZ id x y z`; `EDGE_PROJECT_P2SC` / `EDGE_P2SC point-id cam-id u v u_right` + the six
    upper-triangular values of the information row by row (:1303-1358). The edge's first vertex is the camera, the
    SECOND id (CEdgeP2SC3D, BA_Types.h:724-727). The d of the FILE is the distortion per pixel of radius: the parsed
    vertex multiplies it by 0.5 (fx + fy) (TVertexSCam3D, include/slam/Parser.h:580-587) into the internal d that
    Project_P2SC divides again, and so does this loader -- intr holds the internal value. Returns dict(cams (nc, 6),
    intr (nc, 6), points (np, 3), obs (no, 5) camera INDEX, point INDEX, u v u_right, info (no, 3, 3), cam_id, pt_id: the
    vertex ids, in file order)."""
    from scipy.spatial.transform import Rotation
    cams, pts, edges, info = [], [], [], []
    with open(path) as f:
        for ln in f:
            t = ln.split()
            if not t or t[0].startswith("#") or t[0].startswith("%"):
                continue
            tok, a = t[0].upper(), t[1:]
            if tok == "VERTEX_SCAM" and len(a) >= 14:
                cams.append([float(x) for x in a[:14]])
            elif tok == "VERTEX_XYZ" and len(a) >= 4:
                pts.append([float(x) for x in a[:4]])
            elif tok in _P2SC_EDGE and len(a) >= 11:
                edges.append([float(x) for x in a[:5]])
                info.append(_upper_to_full([float(x) for x in a[5:11]], 3))
    cams_f, pts_f, e = np.array(cams).reshape(-1, 14), np.array(pts).reshape(-1, 4), np.array(edges).reshape(-1, 5)
    q = Rotation.from_quat(cams_f[:, 4:8]).inv()
    cam_id, pt_id = cams_f[:, 0].astype(np.int64), pts_f[:, 0].astype(np.int64)
    nv = int(max(cam_id.max(initial=-1), pt_id.max(initial=-1))) + 1
    cam_index, pt_index = np.full(nv, -1, dtype=np.int64), np.full(nv, -1, dtype=np.int64)
    cam_index[cam_id] = np.arange(cam_id.size)
    pt_index[pt_id] = np.arange(pt_id.size)
    ci, pi = cam_index[e[:, 1].astype(np.int64)], pt_index[e[:, 0].astype(np.int64)]
    if (ci < 0).any() or (pi < 0).any():
        raise ValueError("an EDGE_PROJECT_P2SC line names a vertex that is no VERTEX_SCAM / VERTEX_XYZ: %s" % path)
    intr = cams_f[:, 8:14].copy()
    intr[:, 4] *= 0.5 * (intr[:, 0] + intr[:, 1])   # TVertexSCam3D's constructor (include/slam/Parser.h:580-587)
    return dict(cams=np.concatenate([q.apply(-cams_f[:, 1:4]), q.as_rotvec()], axis=1), intr=intr,
                points=pts_f[:, 1:4].copy(), obs=np.concatenate([ci[:, None].astype(np.float64), pi[:, None].astype(np.float64),
                                                                  e[:, 2:5]], axis=1),
                info=np.array(info).reshape(-1, 3, 3), cam_id=cam_id, pt_id=pt_id)


def stereo_lines(cams, intr, points, obs, info=None, cam_id=None, pt_id=None):
    """the lines of save_stereo_graph: vertices in id order, then the edges as given, everything with %.17g"""
    from scipy.spatial.transform import Rotation
    cams, intr, points, obs = (np.asarray(a, dtype=np.float64) for a in (cams, intr, points, obs))
    nc, npts = cams.shape[0], points.shape[0]
    cam_id = np.arange(nc) if cam_id is None else np.asarray(cam_id)
    pt_id = nc + np.arange(npts) if pt_id is None else np.asarray(pt_id)
    R = Rotation.from_rotvec(cams[:, 3:6])
    C = -R.inv().apply(cams[:, :3])            # camera centre in the world
    q = R.inv().as_quat()                       # x y z w, camera-to-world
    intr_f = intr.copy()
    intr_f[:, 4] /= 0.5 * (intr[:, 0] + intr[:, 1])   # the file holds d per pixel of radius, the reader scales it back
    lines = []
    for v in np.argsort(np.concatenate([cam_id, pt_id]), kind="stable"):
        if v < nc:
            lines.append("VERTEX_SCAM %d " % cam_id[v] + " ".join("%.17g" % x for x in (*C[v], *q[v], *intr_f[v])))
        else:
            lines.append("VERTEX_XYZ %d " % pt_id[v - nc] + " ".join("%.17g" % x for x in points[v - nc]))
    iu = np.triu_indices(3)
    for k, o in enumerate(obs):
        m = np.eye(3) if info is None else np.asarray(info[k])
        lines.append("EDGE_PROJECT_P2SC %d %d " % (pt_id[int(o[1])], cam_id[int(o[0])]) +
                     " ".join("%.17g" % x for x in (*o[2:5], *m[iu])))
    return lines


def save_stereo_graph(path, cams, intr, points, obs, info=None, cam_id=None, pt_id=None):
    """Stereo BA graph in the reference's text format (tokens: load_stereo_graph). cams (nc, 6) world-to-camera [t |
    axis-angle] (the reference's internal CVertexSCam state; the file gets centre + camera-to-world quaternion), intr
    (nc, 6) fx fy cx cy d b (d the internal value; the file gets d / (0.5 (fx + fy))), points (np, 3), obs (no, 5)
    camera index, point index, u v u_right (written point id first, as the parser wants), info (no, 3, 3) or None
    (identity); cam_id / pt_id: vertex ids (default: cameras 0..nc-1, points nc..). Vertices are written in id order."""
    with open(path, "w") as f:
        f.write("\n".join(stereo_lines(cams, intr, points, obs, info, cam_id, pt_id)) + "\n")


# --------------------------------------------------------------------------------------------------
# self-calibrating bundle adjustment: cameras CVertexCam (6), points CVertexXYZ (3), intrinsics CVertexIntrinsics (5),
# one ternary edge CEdgeP2CI3D per observation (include/slam/BA_Types.h:141-206, 562-700)
# --------------------------------------------------------------------------------------------------
_P2CI_EDGE = {"EDGE_PROJECT_P2MCI", "EDGE_P2MCI", "EDGE_P2CI"}   # ParsePrimitives.h:1252-1254
BAI_INTR_WIDTH = 6   # width of an intrinsics vertex inside the library: 5 live coordinates + 1 inert


def bai_expectation(cam, intr, X):
    """CBAJacobians::Project_P2C (include/slam/BASolverBase.h:260-327) as the reference writes it, one row per observation:
    cam (k, 6) [t | axis-angle] world -> camera, intr (k, 5) fx fy cx cy kappa, X (k, 3) -> (k, 2). x = R X + t,
    uv = A x / (A x)_2, k = kappa / (0.5 (fx + fy)), r = |uv - c|, uv <- c + (1 + r r k)(uv - c)."""
    from scipy.spatial.transform import Rotation
    cam, intr, X = (np.asarray(a, dtype=np.float64) for a in (cam, intr, X))
    R = Rotation.from_rotvec(cam[:, 3:6]).as_matrix()
    fx, fy, cx, cy = (intr[:, i] for i in range(4))
    k = intr[:, 4] / (0.5 * (fx + fy))
    c = np.stack([cx, cy], axis=1)
    x = np.einsum("eij,ej->ei", R, X) + cam[:, :3]
    uv = np.stack([fx * x[:, 0] + cx * x[:, 2], fy * x[:, 1] + cy * x[:, 2]], axis=1) / x[:, 2:3]
    r = np.sqrt(((uv - c) ** 2).sum(axis=1))
    return c + (1 + r * r * k)[:, None] * (uv - c)


def bai_ids(nc, npts, ni, cam_id=None, pt_id=None, intr_id=None):
    """default vertex ids: intrinsics 0..ni-1, cameras after them, points last"""
    intr_id = np.arange(ni) if intr_id is None else np.asarray(intr_id, dtype=np.int64)
    cam_id = ni + np.arange(nc) if cam_id is None else np.asarray(cam_id, dtype=np.int64)
    pt_id = ni + nc + np.arange(npts) if pt_id is None else np.asarray(pt_id, dtype=np.int64)
    return cam_id, pt_id, intr_id


def bai_linearize(cams, intr, points, obs, cam_id=None, pt_id=None, intr_id=None, info=None):
    """Hot-path inputs (synth.Problem) of a bundle adjustment with intrinsics vertices at the given estimate: the float64
    mirror of spp_ba_intrinsics_linearize_device. cams (nc, 6) [t | axis-angle] world -> camera, intr (ni, 5) fx fy cx cy
    kappa, points (np, 3), obs (no, 5) camera index, point index, intrinsics index, u v; info (no, 2, 2) or None (identity).
    r = z - uv with the projection of CBAJacobians::Project_P2C (BASolverBase.h:260-327); J0, J1 as ba_linearize (the camera
    increment of Relative_to_Absolute, the point); J2 w.r.t. the plain increment of Relative_to_Absolute_Intrinsics
    (:204-212), analytic where the reference takes forward differences (:690-759): with p = (x0/x2, x1/x2), d = (fx p0,
    fy p1), F = fx + fy, k = kappa / (0.5 F), r2 = |d|^2, g = 1 + r2 k:
        d uv / d fx = g (p0, 0) + d (2 k d0 p0 - r2 k / F),  d uv / d fy = g (0, p1) + d (2 k d1 p1 - r2 k / F),
        d uv / d cx = (1, 0),  d uv / d cy = (0, 1),  d uv / d kappa = d r2 / (0.5 F).
    The intrinsics vertex is BAI_INTR_WIDTH = 6 wide here: J2 is (no, 12), 2x6 column-major with a zero last column, and
    dim holds 6 for it. Extra keys of the Problem: v2, d2 = 6, live2 = 5, J2. Vertex ids: bai_ids."""
    from scipy.spatial.transform import Rotation
    from .synth import Problem
    cams, intr, points, obs = (np.asarray(a, dtype=np.float64) for a in (cams, intr, points, obs))
    nc, npts, ni, no = cams.shape[0], points.shape[0], intr.shape[0], obs.shape[0]
    co, po, io = (obs[:, i].astype(np.int64) for i in range(3))
    cam_id, pt_id, intr_id = bai_ids(nc, npts, ni, cam_id, pt_id, intr_id)
    R = Rotation.from_rotvec(cams[:, 3:]).as_matrix()[co]
    X = points[po]
    x = np.einsum("eij,ej->ei", R, X) + cams[co, :3]
    fx, fy, cx, cy, kappa = (intr[io, i] for i in range(5))
    F = fx + fy
    k = kappa / (0.5 * F)
    iz = 1.0 / x[:, 2]
    p = x[:, :2] * iz[:, None]
    d = np.stack([fx * x[:, 0] * iz, fy * x[:, 1] * iz], axis=1)
    r2 = (d ** 2).sum(axis=1)
    g = 1 + r2 * k
    uv = np.stack([cx, cy], axis=1) + g[:, None] * d
    Jd = np.zeros((no, 2, 3))
    Jd[:, 0, 0], Jd[:, 0, 2] = fx * iz, -fx * x[:, 0] * iz * iz
    Jd[:, 1, 1], Jd[:, 1, 2] = fy * iz, -fy * x[:, 1] * iz * iz
    D = g[:, None, None] * np.eye(2)[None] + 2 * k[:, None, None] * np.einsum("ei,ej->eij", d, d)
    PR = np.einsum("eij,ejk,ekl->eil", D, Jd, R)
    J0 = np.concatenate([PR, -np.einsum("eij,ejk->eik", PR, _hat(X))], axis=2)
    kF = r2 * k / F
    sx, sy, sk = 2 * k * d[:, 0] * p[:, 0] - kF, 2 * k * d[:, 1] * p[:, 1] - kF, r2 / (0.5 * F)
    J2 = np.zeros((no, 2, BAI_INTR_WIDTH))
    J2[:, :, 0] = d * sx[:, None]
    J2[:, 0, 0] += g * p[:, 0]
    J2[:, :, 1] = d * sy[:, None]
    J2[:, 1, 1] += g * p[:, 1]
    J2[:, 0, 2] = 1.0
    J2[:, 1, 3] = 1.0
    J2[:, :, 4] = d * sk[:, None]
    dim = np.empty(nc + npts + ni, dtype=np.int32)
    dim[cam_id], dim[pt_id], dim[intr_id] = 6, 3, BAI_INTR_WIDTH
    Om = np.tile(np.eye(2), (no, 1, 1)) if info is None else np.asarray(info, dtype=np.float64)
    return Problem(name="bai", dim=dim, v0=cam_id[co], v1=pt_id[po], v2=intr_id[io], d0=6, d1=3, d2=BAI_INTR_WIDTH, live2=5, rd=2,
                   J0=np.ascontiguousarray(J0.transpose(0, 2, 1)).reshape(no, 12),
                   J1=np.ascontiguousarray(PR.transpose(0, 2, 1)).reshape(no, 6),
                   J2=np.ascontiguousarray(J2.transpose(0, 2, 1)).reshape(no, 12),
                   Om=np.ascontiguousarray(Om).reshape(no, 4), r=obs[:, 3:5] - uv, unary_vertex=0, damping=0.0)


def bai_intrinsics_plus(intr, d):
    """CVertexIntrinsics::Operator_Plus AS WRITTEN (BA_Types.h:170-185), rows of intr (ni, 5) and of the increment d (ni, 5):
    fx fy cx cy plain sums; kappa divided by 0.5 fx fy (the PRODUCT) of the old state, incremented by its delta divided
    alike, multiplied by 0.5 fx fy of the new state."""
    intr, d = np.asarray(intr, dtype=np.float64), np.asarray(d, dtype=np.float64)
    out = intr.copy()
    den = 0.5 * (intr[:, 0] * intr[:, 1])
    dn = intr[:, 4] / den + d[:, 4] / den
    out[:, :4] = intr[:, :4] + d[:, :4]
    out[:, 4] = dn * (0.5 * (out[:, 0] * out[:, 1]))
    return out


def bai_assemble_dense(prob, damping=0.0):
    """float64 mirror of spp_assemble_ternary_device as one dense matrix: Lambda (n, n) and eta (n) of a bai_linearize
    Problem in the padded layout -- J^T Omega J + unary factor (identity on the live coordinates of an intrinsics vertex)
    + damping on every diagonal entry + 1.0 on the inert diagonal entries."""
    dim = np.asarray(prob.dim, dtype=np.int64)
    base = np.concatenate([[0], np.cumsum(dim)])
    n, no = int(base[-1]), prob.v0.size
    lam, eta = np.zeros((n, n)), np.zeros(n)
    Om = prob.Om.reshape(no, 2, 2)
    Js = [(prob.v0, prob.J0.reshape(no, 6, 2).transpose(0, 2, 1)), (prob.v1, prob.J1.reshape(no, 3, 2).transpose(0, 2, 1)),
          (prob.v2, prob.J2.reshape(no, 6, 2).transpose(0, 2, 1))]
    for e in range(no):
        for va, Ja in Js:
            ia = slice(base[va[e]], base[va[e] + 1])
            eta[ia] += Ja[e].T @ (Om[e] @ prob.r[e])
            for vb, Jb in Js:
                lam[ia, slice(base[vb[e]], base[vb[e] + 1])] += Ja[e].T @ Om[e] @ Jb[e]
    is_intr = np.zeros(dim.size, dtype=bool)
    is_intr[prob.v2] = True
    u = prob.unary_vertex
    if u is not None and u >= 0:
        live = 5 if is_intr[u] else int(dim[u])
        lam[base[u] + np.arange(live), base[u] + np.arange(live)] += 1.0
    inert = base[:-1][is_intr] + 5
    lam[inert, inert] += 1.0
    lam[np.arange(n), np.arange(n)] += damping
    return lam, eta


def load_bai_graph(path):
    """A bundle adjustment graph with intrinsics vertices as the reference's parser reads it: `VERTEX_CAM id x y z qx qy qz
    qw fx fy cx cy d` (camera-to-world centre + quaternion, inverted by the parser into the world-to-camera [t |
    axis-angle] it optimizes, include/slam_app/ParsePrimitives.h:861-931; the five intrinsics of the line are not used by
    CEdgeP2CI3D); `VERTEX_XYZ id x y z`; `VERTEX_INTRINSICS id fx fy cx cy d` (:932-976), d the distortion per pixel of radius
    which the parsed vertex multiplies by 0.5 (fx + fy) into the internal kappa (TVertexIntrinsics, include/slam/Parser.h:
    543-549) -- intr holds the internal value; `EDGE_P2CI point-id cam-id intrinsics-id u v xx xy yy` (:1241-1297; the edge's
    vertices are camera, point, intrinsics: BA_Types.h:583-587). Returns dict(cams (nc, 6), intr (ni, 5), points (np, 3),
    obs (no, 5) camera INDEX, point INDEX, intrinsics INDEX, u v, info (no, 2, 2), cam_id, pt_id, intr_id: vertex ids in
    file order)."""
    from scipy.spatial.transform import Rotation
    cams, pts, intrs, edges, info = [], [], [], [], []
    with open(path) as f:
        for ln in f:
            t = ln.split()
            if not t or t[0].startswith("#") or t[0].startswith("%"):
                continue
            tok, a = t[0].upper(), t[1:]
            if tok == "VERTEX_CAM" and len(a) >= 13:
                cams.append([float(x) for x in a[:13]])
            elif tok == "VERTEX_XYZ" and len(a) >= 4:
                pts.append([float(x) for x in a[:4]])
            elif tok == "VERTEX_INTRINSICS" and len(a) >= 6:
                intrs.append([float(x) for x in a[:6]])
            elif tok in _P2CI_EDGE and len(a) >= 8:
                edges.append([float(x) for x in a[:5]])
                info.append(_upper_to_full([float(x) for x in a[5:8]], 2))
    cams_f, pts_f = np.array(cams).reshape(-1, 13), np.array(pts).reshape(-1, 4)
    intr_f, e = np.array(intrs).reshape(-1, 6), np.array(edges).reshape(-1, 5)
    q = Rotation.from_quat(cams_f[:, 4:8]).inv()
    cam_id, pt_id, intr_id = (a[:, 0].astype(np.int64) for a in (cams_f, pts_f, intr_f))
    nv = int(max(cam_id.max(initial=-1), pt_id.max(initial=-1), intr_id.max(initial=-1))) + 1
    index = []
    for ids in (cam_id, pt_id, intr_id):
        ix = np.full(nv, -1, dtype=np.int64)
        ix[ids] = np.arange(ids.size)
        index.append(ix)
    ci, pi, ii = index[0][e[:, 1].astype(np.int64)], index[1][e[:, 0].astype(np.int64)], index[2][e[:, 2].astype(np.int64)]
    if (ci < 0).any() or (pi < 0).any() or (ii < 0).any():
        raise ValueError("an EDGE_P2CI line names a vertex that is no VERTEX_CAM / VERTEX_XYZ / VERTEX_INTRINSICS: %s" % path)
    intr = intr_f[:, 1:6].copy()
    intr[:, 4] *= 0.5 * (intr[:, 0] + intr[:, 1])
    f64 = lambda a: a[:, None].astype(np.float64)
    return dict(cams=np.concatenate([q.apply(-cams_f[:, 1:4]), q.as_rotvec()], axis=1), intr=intr, points=pts_f[:, 1:4].copy(),
                obs=np.concatenate([f64(ci), f64(pi), f64(ii), e[:, 3:5]], axis=1), info=np.array(info).reshape(-1, 2, 2),
                cam_id=cam_id, pt_id=pt_id, intr_id=intr_id)


def bai_lines(cams, intr, points, obs, info=None, cam_id=None, pt_id=None, intr_id=None):
    """the lines of save_bai_graph: vertices in id order, then the edges as given, everything with %.17g. A camera's line
    carries the intrinsics of the vertex its first observation names (the application does not read them)."""
    from scipy.spatial.transform import Rotation
    cams, intr, points, obs = (np.asarray(a, dtype=np.float64) for a in (cams, intr, points, obs))
    nc, npts, ni = cams.shape[0], points.shape[0], intr.shape[0]
    cam_id, pt_id, intr_id = bai_ids(nc, npts, ni, cam_id, pt_id, intr_id)
    R = Rotation.from_rotvec(cams[:, 3:6])
    C = -R.inv().apply(cams[:, :3])
    q = R.inv().as_quat()
    intr_f = intr.copy()
    intr_f[:, 4] /= 0.5 * (intr[:, 0] + intr[:, 1])   # the file holds d per pixel of radius, the reader scales it back
    first = np.zeros(nc, dtype=np.int64)
    co = obs[:, 0].astype(np.int64)
    first[co[::-1]] = obs[::-1, 2].astype(np.int64)
    lines = []
    for v in np.argsort(np.concatenate([cam_id, pt_id, intr_id]), kind="stable"):
        if v < nc:
            lines.append("VERTEX_CAM %d " % cam_id[v] + " ".join("%.17g" % x for x in (*C[v], *q[v], *intr_f[first[v]])))
        elif v < nc + npts:
            lines.append("VERTEX_XYZ %d " % pt_id[v - nc] + " ".join("%.17g" % x for x in points[v - nc]))
        else:
            lines.append("VERTEX_INTRINSICS %d " % intr_id[v - nc - npts] + " ".join("%.17g" % x for x in intr_f[v - nc - npts]))
    for k, o in enumerate(obs):
        m = np.eye(2) if info is None else np.asarray(info[k])
        lines.append("EDGE_P2CI %d %d %d " % (pt_id[int(o[1])], cam_id[int(o[0])], intr_id[int(o[2])]) +
                     " ".join("%.17g" % x for x in (o[3], o[4], m[0, 0], m[0, 1], m[1, 1])))
    return lines


def save_bai_graph(path, cams, intr, points, obs, info=None, cam_id=None, pt_id=None, intr_id=None):
    """Bundle adjustment graph with intrinsics vertices in the reference's text format (tokens: load_bai_graph). cams
    (nc, 6) world-to-camera [t | axis-angle], intr (ni, 5) fx fy cx cy kappa (the internal value; the file gets kappa /
    (0.5 (fx + fy))), points (np, 3), obs (no, 5) camera index, point index, intrinsics index, u v (written point id
    first, as the parser wants), info (no, 2, 2) or None. Vertices are written in id order, in front of the edges."""
    with open(path, "w") as f:
        f.write("\n".join(bai_lines(cams, intr, points, obs, info, cam_id, pt_id, intr_id)) + "\n")


# --------------------------------------------------------------------------------------------------
# range-only constant-velocity SLAM (ROCV): receivers [p | v] (6) + transmitters (3); constant-velocity edges,
# ranges, transmitter priors (include/slam/ROCV_Types.h, src/slam_app/SolveROCVImpl.cpp)
# --------------------------------------------------------------------------------------------------
_ROCV_TOKENS = {"ROCV:TRANSMITTER", "ROCV:TRANSMITTER_UF", "ROCV:RECEIVER", "ROCV:RECEIVER_GTFAKE", "ROCV:DELTA_TIME",
                "ROCV:RANGE"}   # ParsePrimitives.h:1425, 1443, 1495, 1550, 1604, 1676


def load_rocv_graph(path):
    """A ROCV graph as the reference's parser and edge constructors would build it, line by line
    (include/slam_app/ParsePrimitives.h:1414-1720). Returns
      dim (nv,) 6 for a receiver / 3 for a transmitter, state (flat, laid out by dim), vertex ids 0 .. nv - 1,
      cv (m, 3) i j dt + cv_info (m, 6, 6) + cv_seq (m,) position among all edges of the file,
      rng (k, 3) receiver transmitter range + rng_info (k,) + rng_seq (k,),
      pri (p,) transmitter + pri_info (p, 3, 3) + pri_seq (p,),
      explicit (nv,) the vertex has a ROCV:TRANSMITTER / ROCV:RECEIVER line.
    Lines: ROCV:TRANSMITTER id x y z (CVertexXYZParsePrimitive); ROCV:TRANSMITTER_UF id + the 6 upper-triangular values
    of a 3x3 matrix row by row -- the parser calls them a covariance but hands them to TUnaryFactor3D::m_t_factor and on to
    CEdgeLandmark3DPrior as the information AS GIVEN, nothing is inverted (:1460-1471, Parser.h:412-420, ROCV_Types.h:251-
    252); ROCV:RECEIVER id x y z vx vy vz; ROCV:RECEIVER_GTfake: CIgnoreVertexType (ROCV_Types.h:683-687), skipped;
    ROCV:DELTA_TIME i j dt + the 21 upper-triangular values of the 6x6 information: kept only when i < j, the parser
    prints an error and DROPS a line in the other order (:1638-1656); ROCV:RANGE receiver transmitter range information.
    A vertex an edge meets first is the null vertex (CInitializeNullVertex: zeros), except the second receiver of a
    constant-velocity edge, which starts at (p0 + v0 dt, v0) (CConstVelocity_Initializer, ROCV_Types.h:365-371)."""
    state, dimof, explicit = {}, {}, set()
    cv, cv_info, cv_seq, rng, rng_info, rng_seq, pri, pri_info, pri_seq = [], [], [], [], [], [], [], [], []
    n_edges = 0

    def null(v, d):
        if v not in state:
            state[v], dimof[v] = np.zeros(d), d

    with open(path) as f:
        for ln in f:
            t = ln.split()
            if not t or t[0].startswith("#") or t[0].startswith("%"):
                continue
            tok, a = t[0].upper(), t[1:]
            if tok == "ROCV:TRANSMITTER" and len(a) >= 4:
                v = int(a[0])
                state[v], dimof[v] = np.array([float(x) for x in a[1:4]]), 3
                explicit.add(v)
            elif tok == "ROCV:RECEIVER" and len(a) >= 7:
                v = int(a[0])
                state[v], dimof[v] = np.array([float(x) for x in a[1:7]]), 6
                explicit.add(v)
            elif tok == "ROCV:TRANSMITTER_UF" and len(a) >= 7:
                v = int(a[0])
                null(v, 3)
                pri.append(v)
                pri_info.append(_upper_to_full([float(x) for x in a[1:7]], 3))
                pri_seq.append(n_edges)
                n_edges += 1
            elif tok == "ROCV:DELTA_TIME" and len(a) >= 24:
                i, j, dt = int(a[0]), int(a[1]), float(a[2])
                if not i < j:
                    continue   # "edges are in switched order": the parser ignores the line
                null(i, 6)
                if j not in state:
                    state[j], dimof[j] = np.concatenate([state[i][:3] + state[i][3:] * dt, state[i][3:]]), 6
                cv.append([i, j, dt])
                cv_info.append(_upper_to_full([float(x) for x in a[3:24]], 6))
                cv_seq.append(n_edges)
                n_edges += 1
            elif tok == "ROCV:RANGE" and len(a) >= 4:
                i, j = int(a[0]), int(a[1])
                null(i, 6)
                null(j, 3)
                rng.append([i, j, float(a[2])])
                rng_info.append(float(a[3]))
                rng_seq.append(n_edges)
                n_edges += 1
    nv = max(state) + 1 if state else 0
    if sorted(state) != list(range(nv)):
        raise ValueError("vertex ids are not 0 .. n-1: %s" % path)
    for grp, col, d in ((cv, 0, 6), (cv, 1, 6), (rng, 0, 6), (rng, 1, 3)):
        if any(dimof[int(e[col])] != d for e in grp):
            raise ValueError("an edge joins vertices of the wrong widths: %s" % path)
    if any(dimof[v] != 3 for v in pri):
        raise ValueError("a prior on a vertex that is not a transmitter: %s" % path)
    dim = np.array([dimof[v] for v in range(nv)], dtype=np.int32)
    return dict(dim=dim, state=np.concatenate([state[v] for v in range(nv)]) if nv else np.zeros(0),
                cv=np.array(cv).reshape(-1, 3), cv_info=np.array(cv_info).reshape(-1, 6, 6),
                cv_seq=np.array(cv_seq, dtype=np.int64), rng=np.array(rng).reshape(-1, 3),
                rng_info=np.array(rng_info, dtype=np.float64), rng_seq=np.array(rng_seq, dtype=np.int64),
                pri=np.array(pri, dtype=np.int64), pri_info=np.array(pri_info).reshape(-1, 3, 3),
                pri_seq=np.array(pri_seq, dtype=np.int64),
                explicit=np.isin(np.arange(nv), sorted(explicit)))


def rocv_lines(dim, state, cv, cv_info, rng, rng_info, pri, pri_info, cv_seq=None, rng_seq=None, pri_seq=None, explicit=None,
               ids=None):
    """the lines of a ROCV graph file, everything with %.17g: the edges in the global order and, in front of the first edge
    that touches it, the vertex line of every vertex listed in `explicit` (default: every vertex); the lines of listed
    vertices that no edge touches come last. A receiver without a line must be met first as the second vertex of a
    constant-velocity edge for the file to bring its state back (CConstVelocity_Initializer). ids: vertex id -> id
    written (the application wants ids to appear in increasing order)."""
    dim = np.asarray(dim)
    base = slam2d_offsets(dim)
    cv, rng, pri = np.asarray(cv, dtype=np.float64).reshape(-1, 3), np.asarray(rng, dtype=np.float64).reshape(-1, 3), np.asarray(pri)
    m, k, p = len(cv), len(rng), len(pri)
    cv_seq = np.arange(m) if cv_seq is None else np.asarray(cv_seq)
    rng_seq = m + np.arange(k) if rng_seq is None else np.asarray(rng_seq)
    pri_seq = m + k + np.arange(p) if pri_seq is None else np.asarray(pri_seq)
    explicit = np.ones(dim.size, dtype=bool) if explicit is None else np.asarray(explicit, dtype=bool)
    name = (lambda v: int(v)) if ids is None else (lambda v: ids[int(v)])
    num = lambda xs: " ".join("%.17g" % x for x in xs)
    edges = [None] * (m + k + p)
    for e in range(m):
        edges[cv_seq[e]] = (cv[e, :2], "ROCV:DELTA_TIME %d %d %s %s" % (
            name(cv[e, 0]), name(cv[e, 1]), num(cv[e, 2:3]), num(np.asarray(cv_info[e])[np.triu_indices(6)])))
    for e in range(k):
        edges[rng_seq[e]] = (rng[e, :2], "ROCV:RANGE %d %d %s" % (name(rng[e, 0]), name(rng[e, 1]), num([rng[e, 2], rng_info[e]])))
    for e in range(p):
        edges[pri_seq[e]] = (pri[e:e + 1], "ROCV:TRANSMITTER_UF %d %s" % (name(pri[e]), num(np.asarray(pri_info[e])[np.triu_indices(3)])))
    lines, done = [], np.zeros(dim.size, dtype=bool)

    def vertex_line(u):
        if explicit[u] and not done[u]:
            lines.append("%s %d %s" % ("ROCV:TRANSMITTER" if dim[u] == 3 else "ROCV:RECEIVER", name(u), num(state[base[u]:base[u + 1]])))
        done[u] = True

    for vs, ln in edges:
        for u in vs:
            vertex_line(int(u))
        lines.append(ln)
    for u in range(dim.size):
        vertex_line(u)
    return lines


def save_rocv_graph(path, dim, state, cv, cv_info, rng, rng_info, pri, pri_info, cv_seq=None, rng_seq=None, pri_seq=None,
                    explicit=None):
    """rocv_lines to a file: load_rocv_graph brings every array back bit for bit"""
    with open(path, "w") as f:
        f.write("\n".join(rocv_lines(dim, state, cv, cv_info, rng, rng_info, pri, pri_info, cv_seq, rng_seq, pri_seq,
                                     explicit)) + "\n")


def rocv_range_model(p, l, z):
    """CEdgePosVel_Landmark3D<false> (ROCV_Types.h:163-205) for receiver positions p (k, 3), transmitters l (k, 3), ranges
    z (k,): e = |p - l| from the differences (the reference's Jacobians divide by the square root of the expanded
    polynomial, which cancels), r = z - e, J0 = [(p - l)^T / e | 0 0 0], J1 = -J0[0:3]; at e = 0 both Jacobians are exact
    zeros and r = z (the reference divides 0 by 0). Returns J0 (k, 6), J1 (k, 3), r (k,)."""
    d = p - l
    e = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    u = np.divide(d, e[:, None], out=np.zeros_like(d), where=e[:, None] > 0)
    return np.concatenate([u, np.zeros_like(u)], axis=1), -u, z - e


def rocv_cv_model(x0, x1, dt):
    """CEdgeConstVelocity3D<false> (ROCV_Types.h:543-614) for receivers x0, x1 (m, 6) and time steps dt (m,): expectation
    (p0 + v0 dt, v0), r = -(x1 - expectation), J0 = -[I, dt I; 0, I], J1 = I. Returns J0, J1 (m, 6, 6), r (m, 6)."""
    m = dt.size
    r = -(x1 - np.concatenate([x0[:, :3] + x0[:, 3:] * dt[:, None], x0[:, 3:]], axis=1))
    J0 = np.tile(-np.eye(6), (m, 1, 1))
    J0[:, np.arange(3), 3 + np.arange(3)] = -dt[:, None]
    return J0, np.tile(np.eye(6), (m, 1, 1)), r


def rocv_linearize(dim, state, cv, cv_info, rng, rng_info, pri, pri_info):
    """The three edge groups of a ROCV graph at `state` (flat, laid out by dim), as synth.Problems over the SAME vertices:
    constant velocity (6, 6, 6), ranges (6, 3, 1) and the transmitter priors, a UNARY group (d0, rd) = (3, 3) with v1 None,
    d1 0 and an empty J1: J = I and r = 0 whatever the state (CEdgeLandmark3DPrior::Calculate_Jacobian_Expectation_Error,
    ROCV_Types.h:302-310 -- the prior adds its information to the transmitter's diagonal block, nothing to eta, and its
    chi2 is 0). No built-in unary factor: unary_vertex = -1 (CNullUnaryFactorFactory, SolveROCVImpl.cpp:42-43)."""
    from .synth import Problem
    dim = np.asarray(dim, dtype=np.int32)
    x = np.asarray(state, dtype=np.float64)
    base = slam2d_offsets(dim)
    cv = np.asarray(cv, dtype=np.float64).reshape(-1, 3)
    rng = np.asarray(rng, dtype=np.float64).reshape(-1, 3)
    pri = np.asarray(pri, dtype=np.int64).ravel()
    a, b = cv[:, 0].astype(np.int64), cv[:, 1].astype(np.int64)
    J0, J1, r = rocv_cv_model(x[base[a][:, None] + np.arange(6)], x[base[b][:, None] + np.arange(6)], cv[:, 2])
    m = a.size
    g_cv = Problem(name="rocv_const_velocity", dim=dim, v0=a, v1=b, d0=6, d1=6, rd=6,
                   J0=np.ascontiguousarray(J0.transpose(0, 2, 1)).reshape(m, 36),
                   J1=np.ascontiguousarray(J1.transpose(0, 2, 1)).reshape(m, 36),
                   Om=np.asarray(cv_info, dtype=np.float64).reshape(m, 36), r=r, unary_vertex=-1, damping=0.0)
    vr, vt = rng[:, 0].astype(np.int64), rng[:, 1].astype(np.int64)
    k = vr.size
    H0, H1, rr = rocv_range_model(x[base[vr][:, None] + np.arange(3)], x[base[vt][:, None] + np.arange(3)], rng[:, 2])
    g_rng = Problem(name="rocv_ranges", dim=dim, v0=vr, v1=vt, d0=6, d1=3, rd=1, J0=H0.reshape(k, 6), J1=H1.reshape(k, 3),
                    Om=np.asarray(rng_info, dtype=np.float64).reshape(k, 1), r=rr.reshape(k, 1), unary_vertex=-1, damping=0.0)
    p = pri.size
    g_pri = Problem(name="rocv_priors", dim=dim, v0=pri, v1=None, d0=3, d1=0, rd=3, J0=np.tile(np.eye(3).ravel(), (p, 1)),
                    J1=np.zeros((p, 0)), Om=np.asarray(pri_info, dtype=np.float64).reshape(p, 9), r=np.zeros((p, 3)),
                    unary_vertex=-1, damping=0.0)
    return g_cv, g_rng, g_pri


# --------------------------------------------------------------------------------------------------
# Sim(3) bundle adjustment: cameras CVertexCamSim3 (7: v = [t | w | s] in sim(3)), points CVertexXYZ (3), one binary edge
# CEdgeP2C_XYZ_Sim3_G per observation (include/slam/Sim3_Types.h:178-238, 492-595; CSim3Jacobians, Sim3SolverBase.h).
# The float64 mirror of the device geometry (spp_geometry.hip, the Sim(3) part): the same cells, the same formulas.
# --------------------------------------------------------------------------------------------------
_SIM3_CAM_TOKEN = "VERTEX_CAM:SIM3"                      # include/ba_parameter_acra/Sim3_ParsePrimitives.h:146
_SIM3_EDGE = {"EDGE_PROJECT_P2MC", "EDGE_P2MC"}          # what BAOptimizer.cpp:918-983 writes / ParsePrimitives.h
SIM3_SERIES_TERMS = 24
SIM3_SERIES_Z2 = 1.0      # s^2 + theta^2 below which a, b, c come from the Taylor series
SIM3_SINC_THETA = 1e-4    # theta below which sin(theta) / theta and (1 - cos(theta)) / theta^2 come from two terms


def _sim3_sinc(th):
    """S = sin(th) / th, C = (1 - cos(th)) / th^2, cos(th / 2), sin(th / 2) / th"""
    th = np.asarray(th, dtype=np.float64)
    small = th < SIM3_SINC_THETA
    t = np.where(small, 1.0, th)
    sh, ch = np.sin(0.5 * t), np.cos(0.5 * t)
    so = sh / t
    th2 = th * th
    return (np.where(small, 1.0 - th2 * (1.0 / 6.0), 2.0 * so * ch), np.where(small, 0.5 - th2 * (1.0 / 24.0), 2.0 * so * so),
            np.where(small, 1.0 - th2 * 0.125, ch), np.where(small, 0.5 - th2 * (1.0 / 48.0), so))


def sim3_abc(s, th):
    """a, b, c of V = a I + b [w]x + c [w]x^2 (t_Exp, Sim3SolverBase.h:3867-3898) at scale logarithm s and angle th = |w|:
    a = phi(s), b = Im phi(z) / th, c = (a - Re phi(z)) / th^2, phi(z) = (e^z - 1) / z, z = s + i th. Taylor series for
    |z|^2 < 1 (no division), closed form beyond; returns (a, b, c, cell) with cell 0 = series, 1 = closed form."""
    s, th = np.broadcast_arrays(np.asarray(s, dtype=np.float64), np.asarray(th, dtype=np.float64))
    th2 = th * th
    z2 = s * s + th2
    a = np.where(s == 0.0, 1.0, np.expm1(s) / np.where(s == 0.0, 1.0, s))
    p, q, sn, f = np.zeros_like(z2), np.zeros_like(z2), np.ones_like(z2), 1.0
    bs, cs = np.zeros_like(z2), np.zeros_like(z2)
    with np.errstate(over="ignore", invalid="ignore"):     # (the lanes of the other cell may overflow: not used)
        for n in range(SIM3_SERIES_TERMS):
            f = f / (n + 1)
            bs = bs + p * f
            cs = cs + q * f
            p, q, sn = s * p + sn - th2 * q, s * q + p, sn * s
        E = np.exp(s)
        S, C, _, _ = _sim3_sinc(th)
        zz = np.where(z2 == 0.0, 1.0, z2)
        bc = (s * (E * S - a) + E * th2 * C) / zz
        cc = (a - E * (S - s * C)) / zz
    series = z2 < SIM3_SERIES_Z2
    return a, np.where(series, bs, bc), np.where(series, cs, cc), np.where(series, 0, 1)


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def sim3_exp(v):
    """T = Exp(v), v (n, 7) [t | w | s]: R (n, 3, 3), tau (n, 3), E = e^s (n,), q (n, 4) the unit quaternion (w, x, y, z)
    of R with w >= 0 (CSim3Jacobians::t_Exp, Sim3SolverBase.h:3829-3905)"""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 7)
    t, w, s = v[:, :3], v[:, 3:6], v[:, 6]
    th = np.sqrt((w * w).sum(axis=1))
    S, C, ch, so = _sim3_sinc(th)
    a, b, c, _ = sim3_abc(s, th)
    K = _hat(w)
    R = np.eye(3)[None] + S[:, None, None] * K + C[:, None, None] * np.einsum("eij,ejk->eik", K, K)
    wt = _cross(w, t)
    tau = a[:, None] * t + b[:, None] * wt + c[:, None] * _cross(w, wt)
    sg = np.where(ch < 0, -1.0, 1.0)
    q = np.concatenate([(sg * ch)[:, None], (sg * so)[:, None] * w], axis=1)
    return R, tau, np.exp(s), q


def _quat_mul(p, q):
    return np.stack([p[:, 0] * q[:, 0] - p[:, 1] * q[:, 1] - p[:, 2] * q[:, 2] - p[:, 3] * q[:, 3],
                     p[:, 0] * q[:, 1] + p[:, 1] * q[:, 0] + p[:, 2] * q[:, 3] - p[:, 3] * q[:, 2],
                     p[:, 0] * q[:, 2] - p[:, 1] * q[:, 3] + p[:, 2] * q[:, 0] + p[:, 3] * q[:, 1],
                     p[:, 0] * q[:, 3] + p[:, 1] * q[:, 2] - p[:, 2] * q[:, 1] + p[:, 3] * q[:, 0]], axis=1)


def _quat_to_aa(q):
    q = np.where(q[:, :1] < 0, -q, q)
    vn = np.sqrt((q[:, 1:] ** 2).sum(axis=1))
    scale = np.where(vn < 1e-12, 2.0, 2.0 * np.arctan2(vn, q[:, 0]) / np.where(vn < 1e-12, 1.0, vn))
    return q[:, 1:] * scale[:, None]


def sim3_log(q, tau, s):
    """the inverse of sim3_exp (v_Log, Sim3SolverBase.h:3740-3819): q (n, 4) unit quaternions (w, x, y, z), tau (n, 3), s (n,)
    the LOGARITHM of the scale. V^-1 in closed form: (1 / a) I - (b / D) [w]x + ((b^2 - A c) / (a D)) [w]x^2, A = a - c th^2,
    D = A^2 + th^2 b^2."""
    w = _quat_to_aa(np.asarray(q, dtype=np.float64))
    th2 = (w * w).sum(axis=1)
    a, b, c, _ = sim3_abc(s, np.sqrt(th2))
    A = a - c * th2
    D = A * A + th2 * b * b
    wt = _cross(w, tau)
    t = (1.0 / a)[:, None] * tau + (-b / D)[:, None] * wt + ((b * b - A * c) / (a * D))[:, None] * _cross(w, wt)
    return np.concatenate([t, w, np.asarray(s, dtype=np.float64)[:, None]], axis=1)


def sim3_from_trs(trs):
    """the parser's conversion (Sim3_ParsePrimitives.h:259-263): a file pose [translation | axis-angle | PLAIN scale]
    (TSim3::from_tRs_vector) -> its logarithm, the 7-vector the vertex holds"""
    trs = np.asarray(trs, dtype=np.float64).reshape(-1, 7)
    w = trs[:, 3:6]
    th = np.sqrt((w * w).sum(axis=1))
    _, _, ch, so = _sim3_sinc(th)
    sg = np.where(ch < 0, -1.0, 1.0)
    q = np.concatenate([(sg * ch)[:, None], (sg * so)[:, None] * w], axis=1)
    return sim3_log(q, trs[:, :3], np.log(trs[:, 6]))


def sim3_to_trs(cams):
    """a vertex state -> the file's pose [translation | axis-angle | plain scale] (Exp; the axis-angle is the state's own)"""
    cams = np.asarray(cams, dtype=np.float64).reshape(-1, 7)
    _, tau, E, _ = sim3_exp(cams)
    return np.concatenate([tau, cams[:, 3:6], E[:, None]], axis=1)


def sim3_expectation(cam, intr, X):
    """CSim3Jacobians::Project_P2C_XYZ (Sim3SolverBase.h:630-681), one row per observation: x = e^-s R^T (X - tau),
    k = intr[4] / (0.5 fx fy), uv = c + (1 + |p - c|^2 k)(p - c). Returns (uv, x, R, 1 / E)."""
    R, tau, E, _ = sim3_exp(cam)
    iE = 1.0 / E
    x = iE[:, None] * np.einsum("eji,ej->ei", R, X - tau)
    fx, fy = intr[:, 0], intr[:, 1]
    iz = 1.0 / x[:, 2]
    d = np.stack([fx * x[:, 0] * iz, fy * x[:, 1] * iz], axis=1)
    g = 1.0 + (d ** 2).sum(axis=1) * (intr[:, 4] / (0.5 * (fx * fy)))
    return intr[:, 2:4] + g[:, None] * d, x, R, iE


def sim3_ba_linearize(cams, intr, points, obs, cam_id=None, pt_id=None, info=None):
    """Hot-path inputs (synth.Problem, one (7, 3, 2) group, camera first) of a Sim(3) bundle adjustment: cams (nc, 7)
    [t | w | s], intr (nc, 5) fx fy cx cy d (d the internal value), points (np, 3), obs (no, 4) camera index, point index,
    u v. Jacobians analytic w.r.t. the post-multiplicative camera increment T Exp(delta) and the additive point increment:
    d x / d delta = [-I | [x]x | -x] (the scale column of J0 is identically zero), d x / d X = e^-s R^T."""
    from .synth import Problem
    cams, intr, points, obs = (np.asarray(a, dtype=np.float64) for a in (cams, intr, points, obs))
    nc, npts, no = cams.shape[0], points.shape[0], obs.shape[0]
    co, po = obs[:, 0].astype(np.int64), obs[:, 1].astype(np.int64)
    cam_id = np.arange(nc) if cam_id is None else np.asarray(cam_id)
    pt_id = nc + np.arange(npts) if pt_id is None else np.asarray(pt_id)
    itr = intr[co]
    uv, x, R, iE = sim3_expectation(cams[co], itr, points[po])
    fx, fy = itr[:, 0], itr[:, 1]
    k = itr[:, 4] / (0.5 * (fx * fy))
    iz = 1.0 / x[:, 2]
    d = np.stack([fx * x[:, 0] * iz, fy * x[:, 1] * iz], axis=1)
    g = 1.0 + (d ** 2).sum(axis=1) * k
    Jd = np.zeros((no, 2, 3))
    Jd[:, 0, 0], Jd[:, 0, 2] = fx * iz, -fx * x[:, 0] * iz * iz
    Jd[:, 1, 1], Jd[:, 1, 2] = fy * iz, -fy * x[:, 1] * iz * iz
    D = g[:, None, None] * np.eye(2)[None] + 2 * k[:, None, None] * np.einsum("ei,ej->eij", d, d)
    P = np.einsum("eij,ejk->eik", D, Jd)
    J0 = np.concatenate([-P, np.einsum("eij,ejk->eik", P, _hat(x)), np.zeros((no, 2, 1))], axis=2)
    J1 = iE[:, None, None] * np.einsum("eij,ekj->eik", P, R)
    dim = np.empty(nc + npts, dtype=np.int32)
    dim[cam_id] = 7
    dim[pt_id] = 3
    Om = np.tile(np.eye(2).ravel(), (no, 1)) if info is None else np.ascontiguousarray(info, dtype=np.float64).reshape(no, 4)
    return Problem(name="sim3_ba", dim=dim, v0=cam_id[co], v1=pt_id[po], d0=7, d1=3, rd=2,
                   J0=np.ascontiguousarray(J0.transpose(0, 2, 1)).reshape(no, 14),
                   J1=np.ascontiguousarray(J1.transpose(0, 2, 1)).reshape(no, 6),
                   Om=Om, r=obs[:, 2:4] - uv, unary_vertex=-1, damping=0.0)


def sim3_plus(cams, dx):
    """camera (+) dx of CVertexCamSim3::Operator_Plus: Log(Exp(cam) Exp(dx)) (Relative_to_Absolute, Sim3SolverBase.h:435-452)"""
    cams, dx = np.asarray(cams, dtype=np.float64).reshape(-1, 7), np.asarray(dx, dtype=np.float64).reshape(-1, 7)
    R1, t1, E1, q1 = sim3_exp(cams)
    _, t2, _, q2 = sim3_exp(dx)
    tau = t1 + E1[:, None] * np.einsum("eij,ej->ei", R1, t2)
    return sim3_log(_quat_mul(q1, q2), tau, cams[:, 6] + dx[:, 6])


def load_sim3_graph(path):
    """A Sim(3) BA graph as the reference's parser reads it (include/ba_parameter_acra/Sim3_ParsePrimitives.h:135-276):
    `VERTEX_CAM:SIM3 id tx ty tz ax ay az s fx fy cx cy d` holds the pose as translation, axis-angle and PLAIN scale
    (from_tRs_vector); the vertex stores its logarithm (sim3_from_trs) and d times 0.5 (fx + fy) (:125) -- the projection
    later divides by 0.5 fx fy, as written there. `VERTEX_XYZ id x y z`; `EDGE_PROJECT_P2MC point-id cam-id u v` + the three
    upper-triangular values of the information (BAOptimizer.cpp:918-983). Vertex lines may come after the edges that name
    them. Returns dict(cams (nc, 7), cams_trs (nc, 7) the file's numbers, intr (nc, 5), points, obs (no, 4) camera INDEX,
    point INDEX, u v, info (no, 2, 2), cam_id, pt_id: the vertex ids in file order)."""
    cams, pts, edges, info = [], [], [], []
    with open(path) as f:
        for ln in f:
            t = ln.split()
            if not t or t[0].startswith("#") or t[0].startswith("%"):
                continue
            tok, a = t[0].upper(), t[1:]
            if tok == _SIM3_CAM_TOKEN and len(a) >= 13:
                cams.append([float(x) for x in a[:13]])
            elif tok == "VERTEX_XYZ" and len(a) >= 4:
                pts.append([float(x) for x in a[:4]])
            elif tok in _SIM3_EDGE and len(a) >= 7:
                edges.append([float(x) for x in a[:4]])
                info.append(_upper_to_full([float(x) for x in a[4:7]], 2))
    cams_f, pts_f, e = np.array(cams).reshape(-1, 13), np.array(pts).reshape(-1, 4), np.array(edges).reshape(-1, 4)
    cam_id, pt_id = cams_f[:, 0].astype(np.int64), pts_f[:, 0].astype(np.int64)
    nv = int(max(cam_id.max(initial=-1), pt_id.max(initial=-1), e[:, :2].max(initial=-1))) + 1
    cam_index, pt_index = np.full(nv, -1, dtype=np.int64), np.full(nv, -1, dtype=np.int64)
    cam_index[cam_id] = np.arange(cam_id.size)
    pt_index[pt_id] = np.arange(pt_id.size)
    ci, pi = cam_index[e[:, 1].astype(np.int64)], pt_index[e[:, 0].astype(np.int64)]
    if (ci < 0).any() or (pi < 0).any():
        raise ValueError("an EDGE_PROJECT_P2MC line names a vertex that is no VERTEX_CAM:SIM3 / VERTEX_XYZ: %s" % path)
    intr = cams_f[:, 8:13].copy()
    intr[:, 4] *= 0.5 * (intr[:, 0] + intr[:, 1])
    return dict(cams=sim3_from_trs(cams_f[:, 1:8]), cams_trs=cams_f[:, 1:8].copy(), intr=intr, points=pts_f[:, 1:4].copy(),
                obs=np.concatenate([ci[:, None].astype(np.float64), pi[:, None].astype(np.float64), e[:, 2:4]], axis=1),
                info=np.array(info).reshape(-1, 2, 2), cam_id=cam_id, pt_id=pt_id)


def sim3_lines(cams_trs, intr, points, obs, info=None, cam_id=None, pt_id=None):
    """the lines of save_sim3_graph: every vertex line in front of the first edge that names it (else in id order behind
    the edges), the edges as given, everything with %.17g"""
    cams_trs, intr, points, obs = (np.asarray(a, dtype=np.float64) for a in (cams_trs, intr, points, obs))
    nc, npts = cams_trs.shape[0], points.shape[0]
    cam_id = np.arange(nc) if cam_id is None else np.asarray(cam_id)
    pt_id = nc + np.arange(npts) if pt_id is None else np.asarray(pt_id)
    intr_f = intr.copy()
    intr_f[:, 4] /= 0.5 * (intr[:, 0] + intr[:, 1])   # the file holds d per pixel of radius, the reader scales it back
    cam_line = lambda c: "VERTEX_CAM:SIM3 %d " % cam_id[c] + " ".join("%.17g" % x for x in (*cams_trs[c], *intr_f[c]))
    pt_line = lambda p: "VERTEX_XYZ %d " % pt_id[p] + " ".join("%.17g" % x for x in points[p])
    lines, cam_done, pt_done = [], np.zeros(nc, dtype=bool), np.zeros(npts, dtype=bool)
    iu = np.triu_indices(2)
    for k, o in enumerate(obs):
        c, p = int(o[0]), int(o[1])
        if not cam_done[c]:
            lines.append(cam_line(c))
            cam_done[c] = True
        if not pt_done[p]:
            lines.append(pt_line(p))
            pt_done[p] = True
        m = np.eye(2) if info is None else np.asarray(info[k])
        lines.append("EDGE_PROJECT_P2MC %d %d " % (pt_id[p], cam_id[c]) + " ".join("%.17g" % x for x in (*o[2:4], *m[iu])))
    rest = [(cam_id[c], cam_line(c)) for c in np.flatnonzero(~cam_done)] + [(pt_id[p], pt_line(p)) for p in np.flatnonzero(~pt_done)]
    return lines + [ln for _, ln in sorted(rest)]


def save_sim3_graph(path, cams_trs, intr, points, obs, info=None, cam_id=None, pt_id=None):
    """Sim(3) BA graph in the reference's text format (tokens: load_sim3_graph). cams_trs (nc, 7): the poses as the FILE
    holds them, [translation | axis-angle | plain scale] (sim3_to_trs of a vertex state); intr (nc, 5) with d the internal
    value (the file gets d / (0.5 (fx + fy))); obs (no, 4) camera index, point index, u v (written point id first)."""
    with open(path, "w") as f:
        f.write("\n".join(sim3_lines(cams_trs, intr, points, obs, info, cam_id, pt_id)) + "\n")
