"""The geometry of slam_plus_plus_amd/csrc/spp_geometry.hip at 50 digits (mpmath, host only).

Part 1 -- the MODELS, written from the model definitions in the header comments of spp_geometry.hip and formats.py, never
from the analytic Jacobians: exp / log on SO(3) (log gives the w >= 0 representative), Relative_to_Absolute (t + R dt,
R exp(dr)), Absolute_to_Relative and the CEdgePose3D error, R^T (l - t), the 2D relative pose with its fmod clamps, the
range-bearing observation with its 1e-5 floor, Project_P2C, Project_P2SC in the reference's own two-rotation form. Every
Jacobian is a central difference of these at h = 1e-20 over the increment the kernel documents; results are rounded once to
float64. (One exception, forced by the model itself: below its 1e-5 floor the range-bearing edge's Jacobians are no derivative
of anything -- the reference evaluates its formulas with the floored range -- so there, and only there, the documented formulas
are evaluated at 50 digits with the floored range.)

Part 2 -- the KERNEL FORMS (k_*): the arithmetic of the device functions that hold a threshold (axis_angle_to_rot,
aa_to_quat, quat_to_aa, the Jr^-1 coefficient, the range floor, the rho guards), in mpmath with a switch per threshold, so
that tests/test_geometry_ref_host.py can evaluate BOTH arms at a threshold and measure what the choice does to an output.
"""
import mpmath as mp
import numpy as np

DPS = 50
TH_ROT = 1e-6      # axis_angle_to_rot: series below
TH_QUAT = 1e-12    # aa_to_quat: (1, a / 2) below
TH_VN = 1e-12      # quat_to_aa: scale 2 below
TH_JR = 1e-4       # Jr^-1 coefficient: series below
RB_FLOOR = 1e-5    # range floor of the range-bearing edge


def precise(f):
    """run f at DPS digits whatever the caller's precision"""
    def g(*a, **k):
        with mp.workdps(DPS):
            return f(*a, **k)
    g.__name__, g.__doc__ = f.__name__, f.__doc__
    return g


def V(a):
    """float64 -> mpf, exactly"""
    return [x if isinstance(x, mp.mpf) else mp.mpf(float(x)) for x in a]


def F(a):
    """mpf -> float64, rounded once"""
    return np.array([float(x) for x in a], dtype=np.float64)


def dot(a, b):
    return mp.fsum(x * y for x, y in zip(a, b))


def norm(a):
    return mp.sqrt(dot(a, a))


def matvec(M, v):
    return [dot(r, v) for r in M]


def matmul(A, B):
    return [[mp.fsum(A[i][k] * B[k][j] for k in range(3)) for j in range(3)] for i in range(3)]


def tr(M):
    return [list(r) for r in zip(*M)]


def hat(v):
    return [[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]]


def eye():
    return [[mp.mpf(int(i == j)) for j in range(3)] for i in range(3)]


# ---------------------------------------------------------------------------------------------------------------------
# part 1: models
# ---------------------------------------------------------------------------------------------------------------------
def so3_exp(a):
    """Rodrigues: I + sin(th)/th K + (1 - cos th)/th^2 K^2, the identity at th = 0"""
    th = norm(a)
    if th == 0:
        return eye()
    K = hat(a)
    K2 = matmul(K, K)
    A, sh = mp.sin(th) / th, mp.sin(th / 2)
    B = 2 * sh * sh / (th * th)   # (1 - cos th) / th^2 without the cancellation
    return [[int(i == j) + A * K[i][j] + B * K2[i][j] for j in range(3)] for i in range(3)]


def so3_log(R):
    """axis-angle of R through the unit quaternion with w >= 0 (angle in [0, pi]); the callers keep R away from pi"""
    w = mp.sqrt(1 + R[0][0] + R[1][1] + R[2][2]) / 2
    v = [(R[2][1] - R[1][2]) / (4 * w), (R[0][2] - R[2][0]) / (4 * w), (R[1][0] - R[0][1]) / (4 * w)]
    vn = norm(v)
    if vn == 0:
        return [mp.mpf(0)] * 3
    s = 2 * mp.atan2(vn, w) / vn
    return [x * s for x in v]




def pose_R(p):
    """[t | axis-angle] -> (t, R)"""
    return list(p[:3]), so3_exp(p[3:6])


def rel_to_abs_R(t, R, d):
    """C3DJacobians::Relative_to_Absolute on (t, R): t + R dt, R exp(dr)"""
    return [a + b for a, b in zip(t, matvec(R, d[:3]))], matmul(R, so3_exp(d[3:6]))




def abs_to_rel_R(t1, R1, t2, R2):
    """C3DJacobians::Absolute_to_Relative: R1^T (t2 - t1), log(R1^T R2)"""
    R1t = tr(R1)
    return matvec(R1t, [a - b for a, b in zip(t2, t1)]) + so3_log(matmul(R1t, R2))


def pose3d_error(z, e):
    """CEdgePose3D: [z_t - e_t ; log(R(z_r) R(e_r)^T)]"""
    return [a - b for a, b in zip(z[:3], e[:3])] + so3_log(matmul(so3_exp(z[3:6]), tr(so3_exp(e[3:6]))))


def landmark_expect_R(t, R, l):
    """C3DJacobians::Absolute_to_Relative_Landmark: R^T (l - t)"""
    return matvec(tr(R), [a - b for a, b in zip(l, t)])


def two_pi():
    return 2 * mp.pi


def fmod_c(x, y):
    """C fmod: x - y trunc(x / y), the sign of x"""
    q = x / y
    n = mp.floor(q) if q >= 0 else mp.ceil(q)
    return x - y * n


def clamp_angle(a):
    """C2DJacobians::f_ClampAngle_2Pi"""
    return fmod_c(a, two_pi())


def clamp_error_arm(e):
    """which of e, e - 2 pi, e + 2 pi f_ClampAngularError_2Pi returns: 0, 1, 2"""
    e = clamp_angle(e)
    a, b = e - two_pi(), e + two_pi()
    m, arm = e, 0
    if abs(a) < abs(m):
        m, arm = a, 1
    if abs(b) < abs(m):
        m, arm = b, 2
    return m, arm




def se2_expect(p1, p2):
    """C2DJacobians::Absolute_to_Relative: the second pose in the frame of the first, angle clamped"""
    c, s = mp.cos(p1[2]), mp.sin(p1[2])
    de, dn = p2[0] - p1[0], p2[1] - p1[1]
    return [c * de + s * dn, -s * de + c * dn, clamp_angle(p2[2] - p1[2])]


def rb_expect_raw(p, l):
    """Observation2D_RangeBearing before its floor: |l - p|, atan2 - pose angle clamped"""
    de, dn = l[0] - p[0], l[1] - p[1]
    return [mp.sqrt(de * de + dn * dn), clamp_angle(mp.atan2(dn, de) - p[2])]


def project_p2c_R(t, R, intr, X):
    """CBAJacobians::Project_P2C: x = R X + t, d = (fx x/z, fy y/z), k' = k / ((fx + fy) / 2), uv = c + (1 + |d|^2 k') d"""
    x = [a + b for a, b in zip(matvec(R, X), t)]
    fx, fy, cx, cy, k = intr[:5]
    kp = k / ((fx + fy) / 2)
    d0, d1 = fx * x[0] / x[2], fy * x[1] / x[2]
    g = 1 + (d0 * d0 + d1 * d1) * kp
    return [cx + g * d0, cy + g * d1]


def _p2sc_one(t, R, intr, Xw):
    x = [a + b for a, b in zip(matvec(R, Xw), t)]
    fx, fy, cx, cy, d = intr[:5]
    k = d / ((fx + fy) / 2)
    u, v = (fx * x[0] + cx * x[2]) / x[2], (fy * x[1] + cy * x[2]) / x[2]   # A x / (A x)_2
    rho = mp.sqrt((u - cx) ** 2 + (v - cy) ** 2)
    return [cx + (1 + rho * k) * (u - cx), cy + (1 + rho * k) * (v - cy)], rho


def project_p2sc_R(t, R, intr, X):
    """CBAJacobians::Project_P2SC as the reference writes it: the right camera sees the point moved by -b (row 0 of R)^T
    through the same rotation, projection and distortion (linear in rho) with its own rho"""
    b = intr[5]
    uv, _ = _p2sc_one(t, R, intr, X)
    uv2, _ = _p2sc_one(t, R, intr, [X[j] - b * R[0][j] for j in range(3)])
    return [uv[0], uv[1], uv2[0]]


def p2sc_rhos(t, R, intr, X):
    b = intr[5]
    return _p2sc_one(t, R, intr, X)[1], _p2sc_one(t, R, intr, [X[j] - b * R[0][j] for j in range(3)])[1]


def cdiff(f, n):
    """central differences at h = 1e-20: the columns d f / d d_j, i.e. the column-major Jacobian, flattened"""
    h = mp.mpf(10) ** -20
    out = []
    for j in range(n):
        d = [mp.mpf(0)] * n
        d[j] = h
        a = f(d)
        d[j] = -h
        b = f(d)
        out += [(x - y) / (2 * h) for x, y in zip(a, b)]
    return out


# ---- canonical quaternions: only to say which SIGN the kernel's products have before it canonicalises them
def quat_canon(a):
    """(cos th/2, sin(th/2) a / th) flipped to w >= 0; the flip flag"""
    th = norm(a)
    if th == 0:
        return [mp.mpf(1), mp.mpf(0), mp.mpf(0), mp.mpf(0)], False
    c, s = mp.cos(th / 2), mp.sin(th / 2) / th
    q = [c, a[0] * s, a[1] * s, a[2] * s]
    return ([-x for x in q], True) if c < 0 else (q, False)


def quat_mul(p, q):
    return [p[0] * q[0] - p[1] * q[1] - p[2] * q[2] - p[3] * q[3],
            p[0] * q[1] + p[1] * q[0] + p[2] * q[3] - p[3] * q[2],
            p[0] * q[2] - p[1] * q[3] + p[2] * q[0] + p[3] * q[1],
            p[0] * q[3] + p[1] * q[2] - p[2] * q[1] + p[3] * q[0]]


def quat_conj(q):
    return [q[0], -q[1], -q[2], -q[3]]


def angle_cell(th):
    """the cell of a rotation argument: 0 th = 0; 1 (0, 1e-12); 2 [1e-12, 0.99e-6); 3 [0.99e-6, 1e-6): just below the
    series threshold; 4 [1e-6, 1.01e-6]: just above; 5 up to pi; 6 (pi, 2 pi]; 7 beyond 2 pi"""
    if th == 0:
        return 0
    for cell, hi in ((1, mp.mpf(TH_QUAT)), (2, mp.mpf(TH_ROT) * mp.mpf("0.99")), (3, mp.mpf(TH_ROT))):
        if th < hi:
            return cell
    if th <= mp.mpf(TH_ROT) * mp.mpf("1.01"):
        return 4
    return 5 if th <= mp.pi else (6 if th <= 2 * mp.pi else 7)


# ---------------------------------------------------------------------------------------------------------------------
# the families: reference outputs + branch records of one case each
# ---------------------------------------------------------------------------------------------------------------------
SE3_BR = ["cell1", "cell2", "cellz", "w_e_neg", "vn_e_tiny", "jr_series", "w_r_neg", "vn_r_tiny"]


@precise
def se3_edge(p1, p2, z):
    """J0, J1 (36 each, column-major), r (6) of the CEdgePose3D edge; aux: th_e, th_r, w of q1^* q2 and of qz qe^* (canonical
    factors, before the product is canonicalised), vn of both; the branch row (SE3_BR)"""
    p1, p2, z = V(p1), V(p2), V(z)
    t1, R1 = pose_R(p1)
    t2, R2 = pose_R(p2)
    e = abs_to_rel_R(t1, R1, t2, R2)
    J0 = cdiff(lambda d: abs_to_rel_R(*rel_to_abs_R(t1, R1, d), t2, R2), 6)
    J1 = cdiff(lambda d: abs_to_rel_R(t1, R1, *rel_to_abs_R(t2, R2, d)), 6)
    r = pose3d_error(z, e)
    q1, q2, qz = quat_canon(p1[3:])[0], quat_canon(p2[3:])[0], quat_canon(z[3:])[0]
    qe = quat_mul(quat_conj(q1), q2)
    qec = quat_conj(qe) if qe[0] >= 0 else [-x for x in quat_conj(qe)]
    qr = quat_mul(qz, qec)
    th_e, th_r = norm(e[3:]), norm(r[3:])
    vn_e, vn_r = norm(qe[1:]), norm(qr[1:])
    br = [angle_cell(norm(p1[3:])), angle_cell(norm(p2[3:])), angle_cell(norm(z[3:])), int(qe[0] < 0),
          int(vn_e < mp.mpf(TH_VN)), int(th_e < mp.mpf(TH_JR)), int(qr[0] < 0), int(vn_r < mp.mpf(TH_VN))]
    return F(J0), F(J1), F(r), F([th_e, th_r, qe[0], qr[0], vn_e, vn_r]), br


XYZ_BR = ["cell"]


@precise
def xyz_edge(p, l, z):
    """J0 (18), J1 (9), r (3) of the CEdgePoseLandmark3D edge; branch row: the cell of the pose's angle"""
    p, l, z = V(p), V(l), V(z)
    t, R = pose_R(p)
    e = landmark_expect_R(t, R, l)
    J0 = cdiff(lambda d: landmark_expect_R(*rel_to_abs_R(t, R, d), l), 6)
    J1 = cdiff(lambda d: landmark_expect_R(t, R, [a + b for a, b in zip(l, d)]), 3)
    return F(J0), F(J1), F([a - b for a, b in zip(z, e)]), [angle_cell(norm(p[3:]))]


BA_BR = ["cell", "k_zero", "on_axis", "behind"]


@precise
def ba_edge(cam, intr, X, z):
    """J0 (12), J1 (6), r (2) of CEdgeP2C3D; aux: the camera-frame point (3), r2 k'"""
    cam, intr, X, z = V(cam), V(intr), V(X), V(z)
    t, R = pose_R(cam)
    uv = project_p2c_R(t, R, intr, X)
    J0 = cdiff(lambda d: project_p2c_R(*rel_to_abs_R(t, R, d), intr, X), 6)
    J1 = cdiff(lambda d: project_p2c_R(t, R, intr, [a + b for a, b in zip(X, d)]), 3)
    x = [a + b for a, b in zip(matvec(R, X), t)]
    d0, d1 = intr[0] * x[0] / x[2], intr[1] * x[1] / x[2]
    r2k = (d0 * d0 + d1 * d1) * intr[4] / ((intr[0] + intr[1]) / 2)
    br = [angle_cell(norm(cam[3:])), int(intr[4] == 0), int(d0 == 0 and d1 == 0), int(x[2] < 0)]
    return F(J0), F(J1), F([a - b for a, b in zip(z, uv)]), F(x + [r2k]), br


STEREO_BR = ["cell", "k_zero", "b_zero", "rho_l_zero", "rho_r_zero", "rho_l_tiny", "behind"]


@precise
def stereo_edge(cam, intr, X, z):
    """J0 (18), J1 (9), r (3) of CEdgeP2SC3D; aux: the camera-frame point (3), rho left, rho right"""
    cam, intr, X, z = V(cam), V(intr), V(X), V(z)
    t, R = pose_R(cam)
    e = project_p2sc_R(t, R, intr, X)
    J0 = cdiff(lambda d: project_p2sc_R(*rel_to_abs_R(t, R, d), intr, X), 6)
    J1 = cdiff(lambda d: project_p2sc_R(t, R, intr, [a + b for a, b in zip(X, d)]), 3)
    x = [a + b for a, b in zip(matvec(R, X), t)]
    rl, rr = p2sc_rhos(t, R, intr, X)
    br = [angle_cell(norm(cam[3:])), int(intr[4] == 0), int(intr[5] == 0), int(rl == 0), int(rr == 0),
          int(0 < rl < mp.mpf(10) ** -10), int(x[2] < 0)]
    return F(J0), F(J1), F([a - b for a, b in zip(z, e)]), F(x + [rl, rr]), br


SE2_BR = ["a1_outside", "a2_outside", "a1_neg", "a2_neg", "err_arm", "near_plus_pi", "near_minus_pi"]


@precise
def se2_edge(p1, p2, z):
    """J0, J1 (9 each), r (3) of CEdgePose2D; the Jacobians over ADDITIVE pose increments, as 2DSolverBase.h has them"""
    p1, p2, z = V(p1), V(p2), V(z)
    h = se2_expect(p1, p2)
    J0 = cdiff(lambda d: se2_expect([a + b for a, b in zip(p1, d)], p2), 3)
    J1 = cdiff(lambda d: se2_expect(p1, [a + b for a, b in zip(p2, d)]), 3)
    ra, arm = clamp_error_arm(z[2] - h[2])
    tol = mp.mpf(10) ** -6
    br = [int(abs(p1[2]) > two_pi()), int(abs(p2[2]) > two_pi()), int(p1[2] < 0), int(p2[2] < 0), arm,
          int(0 < mp.pi - ra < tol), int(0 < ra + mp.pi < tol)]
    return F(J0), F(J1), F([z[0] - h[0], z[1] - h[1], ra]), br


RB_BR = ["floored", "d_zero", "err_arm", "atan_near_cut_pos", "atan_near_cut_neg", "a_outside"]


def rb_formulas(de, dn, d):
    """the Jacobians of Observation2D_RangeBearing as documented (2DSolverBase.h:443-496), at a given (floored) range d"""
    d2 = d * d
    return [-de / d, dn / d2, -dn / d, -de / d2, mp.mpf(0), mp.mpf(-1)], [de / d, -dn / d2, dn / d, de / d2]


@precise
def rb_edge(p, l, z, floor=True):
    """J0 (6: 2 x 3), J1 (4: 2 x 2), r (2) of CEdgePoseLandmark2D; aux: the unfloored range. floor=False: the edge without
    its floor (the other arm of the kernel's choice; at d = 0 it has no finite Jacobian: None)"""
    p, l, z = V(p), V(l), V(z)
    d, hb = rb_expect_raw(p, l)
    below = d < mp.mpf(RB_FLOOR)
    rng = mp.mpf(RB_FLOOR) if (below and floor) else d
    if not below:
        J0 = cdiff(lambda q: rb_expect_raw([a + b for a, b in zip(p, q)], l), 3)
        J1 = cdiff(lambda q: rb_expect_raw(p, [a + b for a, b in zip(l, q)]), 2)
    elif rng == 0:
        J0 = J1 = None
    else:
        J0, J1 = rb_formulas(l[0] - p[0], l[1] - p[1], rng)
    floored = below and floor
    rb, arm = clamp_error_arm(z[1] - hb)
    at = mp.atan2(l[1] - p[1], l[0] - p[0])
    br = [int(floored), int(d == 0), arm, int(mp.pi - at < mp.mpf("1e-3")), int(at + mp.pi < mp.mpf("1e-3")),
          int(abs(p[2]) > two_pi())]
    return (None if J0 is None else F(J0)), (None if J1 is None else F(J1)), F([z[0] - rng, rb]), F([d]), br


PLUS_BR = ["cell_p", "cell_d", "w_neg", "vn_tiny", "d_zero"]


@precise
def plus_case(p, d):
    """p (+) d = Relative_to_Absolute(p, d): out (6), the composite rotation matrix row-major (9); aux: the composite's
    angle, w of the canonical factors' product, vn"""
    p, d = V(p), V(d)
    t, R = rel_to_abs_R(*pose_R(p), d)
    out = t + so3_log(R)
    q = quat_mul(quat_canon(p[3:])[0], quat_canon(d[3:])[0])
    vn = norm(q[1:])
    br = [angle_cell(norm(p[3:])), angle_cell(norm(d[3:])), int(q[0] < 0), int(vn < mp.mpf(TH_VN)), int(all(x == 0 for x in d))]
    return F(out), F([x for row in R for x in row]), F([norm(out[3:]), q[0], vn]), br


@precise
def upd2_case(p, d):
    """CVertexPose2D::Operator_Plus: the sum, the angle clamped"""
    p, d = V(p), V(d)
    return F([p[0] + d[0], p[1] + d[1], clamp_angle(p[2] + d[2])])


# ---------------------------------------------------------------------------------------------------------------------
# part 2: kernel forms. arms: None = the kernel's own choices; a dict may MOVE a threshold ("TH_ROT", "TH_QUAT", "TH_VN",
# "TH_JR": a case between the two values takes the other arm, every other case is untouched) or switch a sign flip off
# ("no_w_flip": quat_to_aa, "no_quat_flip": aa_to_quat, "no_qec_flip": the conjugate in the SE(3) error).
# ---------------------------------------------------------------------------------------------------------------------
def L(a):
    """the kernel forms keep their 50 digits: absdiff() compares them"""
    return list(a)


@precise
def absdiff(a, b):
    """|a - b| entry by entry at 50 digits (a, b: mpf or float64), rounded to float64 at the end"""
    return np.array([float(abs(x - y)) for x, y in zip(V(a), V(b))])


def _thr(arms, name):
    return mp.mpf((arms or {}).get(name, globals()[name]))


def _off(arms, name):
    return bool((arms or {}).get(name, False))


def k_rot(a, arms=None):
    """axis_angle_to_rot: A = sin(th)/th, B = (1 - cos th)/th^2 by series below TH_ROT, closed form above"""
    x, y, z = a
    th = norm(a)
    if th < _thr(arms, "TH_ROT"):
        A, B = 1 - th * th / 6, mp.mpf(1) / 2 - th * th / 24
    else:
        sh = mp.sin(th / 2)
        A, B = mp.sin(th) / th, 2 * sh * sh / (th * th)
    return [[1 - B * (y * y + z * z), B * x * y - A * z, B * x * z + A * y],
            [B * x * y + A * z, 1 - B * (x * x + z * z), B * y * z - A * x],
            [B * x * z - A * y, B * y * z + A * x, 1 - B * (x * x + y * y)]]


def k_aa_to_quat(a, arms=None):
    th = norm(a)
    if th < _thr(arms, "TH_QUAT"):
        c, s = mp.mpf(1), mp.mpf(1) / 2
    else:
        c, s = mp.cos(th / 2), mp.sin(th / 2) / th
        if c < 0 and not _off(arms, "no_quat_flip"):
            c, s = -c, -s
    return [c, a[0] * s, a[1] * s, a[2] * s]


def k_quat_to_aa(q, arms=None):
    w, v = q[0], list(q[1:])
    if w < 0 and not _off(arms, "no_w_flip"):
        w, v = -w, [-x for x in v]
    vn = norm(v)
    s = mp.mpf(2) if vn < _thr(arms, "TH_VN") else 2 * mp.atan2(vn, w) / vn
    return [x * s for x in v]


@precise
def k_se3_edge(p1, p2, z, arms=None):
    """se3_linearize_edge as the kernel evaluates it (analytic Jacobians, rotations through quaternions): J0, J1, r"""
    p1, p2, z = V(p1), V(p2), V(z)
    R1, R2 = k_rot(p1[3:], arms), k_rot(p2[3:], arms)
    R1t = tr(R1)
    et = matvec(R1t, [a - b for a, b in zip(p2[:3], p1[:3])])
    Re = matmul(R1t, R2)
    qe = quat_mul(quat_conj(k_aa_to_quat(p1[3:], arms)), k_aa_to_quat(p2[3:], arms))
    er = k_quat_to_aa(qe, arms)
    qec = quat_conj(qe)
    if qec[0] < 0 and not _off(arms, "no_qec_flip"):
        qec = [-x for x in qec]
    rr = k_quat_to_aa(quat_mul(k_aa_to_quat(z[3:], arms), qec), arms)
    th = norm(er)
    if th < _thr(arms, "TH_JR"):
        c = mp.mpf(1) / 12 + th * th / 720
    else:
        c = 1 / (th * th) - (1 + mp.cos(th)) / (2 * th * mp.sin(th))
    K = hat(er)
    K2 = matmul(K, K)
    Ji = [[int(i == j) + mp.mpf(K[i][j]) / 2 + c * K2[i][j] for j in range(3)] for i in range(3)]
    J0 = [[mp.mpf(0)] * 6 for _ in range(6)]
    J1 = [[mp.mpf(0)] * 6 for _ in range(6)]
    H, JR = hat(et), matmul(Ji, tr(Re))
    for i in range(3):
        J0[i][i] = mp.mpf(-1)
        for j in range(3):
            J0[i][3 + j] = mp.mpf(H[i][j])
            J0[3 + i][3 + j] = -JR[i][j]
            J1[i][j] = Re[i][j]
            J1[3 + i][3 + j] = Ji[i][j]
    col = lambda M: [M[i][j] for j in range(6) for i in range(6)]
    return {"J0": L(col(J0)), "J1": L(col(J1)), "r": L([a - b for a, b in zip(z[:3], et)] + rr)}


@precise
def k_plus(p, d, arms=None):
    """se3_plus as the kernel evaluates it: out, and the rotation matrix of its rotation part"""
    p, d = V(p), V(d)
    R = k_rot(p[3:], arms)
    t = [a + b for a, b in zip(p[:3], matvec(R, d[:3]))]
    aa = k_quat_to_aa(quat_mul(k_aa_to_quat(p[3:], arms), k_aa_to_quat(d[3:], arms)), arms)
    return {"out": L(t + aa), "R": L([x for row in so3_exp(aa) for x in row])}


@precise
def k_xyz_edge(p, l, z, arms=None):
    """se3_xyz_linearize_kernel: J0 = [-I | [e]x], J1 = R^T, r = z - R^T (l - t)"""
    p, l, z = V(p), V(l), V(z)
    R = k_rot(p[3:], arms)
    e = matvec(tr(R), [a - b for a, b in zip(l, p[:3])])
    H = hat(e)
    J0 = [mp.mpf(-int(i == j)) for j in range(3) for i in range(3)] + [mp.mpf(H[i][j]) for j in range(3) for i in range(3)]
    return {"J0": L(J0), "J1": L([R[j][i] for j in range(3) for i in range(3)]), "r": L([a - b for a, b in zip(z, e)])}


@precise
def k_proj_edge(cam, intr, X, z, stereo, arms=None, guard=True):
    """ba_linearize_kernel / ba_stereo_linearize_kernel (the latter in its x - b e0 form): J0, J1, r. guard=False: the
    stereo kernel's n = q / rho WITHOUT its rho > 0 test -- None where that divides by zero"""
    cam, intr, X, z = V(cam), V(intr), V(X), V(z)
    R = k_rot(cam[3:], arms)
    x = [a + b for a, b in zip(matvec(R, X), cam[:3])]
    fx, fy, cx, cy = intr[:4]
    k, iz = intr[4] / ((fx + fy) / 2), 1 / x[2]
    q0, q1 = fx * x[0] * iz, fy * x[1] * iz
    a0, a2, b1, b2 = fx * iz, -fx * x[0] * iz * iz, fy * iz, -fy * x[1] * iz * iz
    if not stereo:
        g = 1 + (q0 * q0 + q1 * q1) * k
        r = [z[0] - (cx + g * q0), z[1] - (cy + g * q1)]
        D00, D01, D11 = g + 2 * k * q0 * q0, 2 * k * q0 * q1, g + 2 * k * q1 * q1
        P = [[D00 * a0, D01 * b1, D00 * a2 + D01 * b2], [D01 * a0, D11 * b1, D01 * a2 + D11 * b2]]
    else:
        xr = x[0] - intr[5]
        s0 = fx * xr * iz
        rho, rhor = mp.sqrt(q0 * q0 + q1 * q1), mp.sqrt(s0 * s0 + q1 * q1)
        g, gr = 1 + rho * k, 1 + rhor * k
        r = [z[0] - (cx + g * q0), z[1] - (cy + g * q1), z[2] - (cx + gr * s0)]
        if not guard and (rho == 0 or rhor == 0):
            return None
        n0, n1 = (q0 / rho, q1 / rho) if rho > 0 else (0, 0)
        m0, m1 = (s0 / rhor, q1 / rhor) if rhor > 0 else (0, 0)
        D00, D01, D11 = g + k * q0 * n0, k * q0 * n1, g + k * q1 * n1
        E0, E1, c2 = gr + k * s0 * m0, k * s0 * m1, -fx * xr * iz * iz
        P = [[D00 * a0, D01 * b1, D00 * a2 + D01 * b2], [D01 * a0, D11 * b1, D01 * a2 + D11 * b2],
             [E0 * a0, E1 * b1, E0 * c2 + E1 * b2]]
    nr = len(P)
    PR = [[mp.fsum(P[i][k_] * R[k_][j] for k_ in range(3)) for j in range(3)] for i in range(nr)]
    Hx = hat(X)
    PH = [[-mp.fsum(PR[i][k_] * Hx[k_][j] for k_ in range(3)) for j in range(3)] for i in range(nr)]
    J1 = [PR[i][j] for j in range(3) for i in range(nr)]
    return {"J0": L(J1 + [PH[i][j] for j in range(3) for i in range(nr)]), "J1": L(J1), "r": L(r)}
