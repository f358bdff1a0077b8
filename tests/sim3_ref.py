"""Sim(3) bundle adjustment at 50 digits (mpmath, host only), on top of tests/geometry_ref.py, written from the definitions:
Exp through the closed forms of a, b, c with the limits taken analytically (CSim3Jacobians::t_Exp, reference
include/slam/Sim3SolverBase.h:3829-3905), Log as its inverse (:3740-3819; V t = tau by an LU at 50 digits), the group
product, Project_P2C_XYZ (:630-681). Jacobians are central differences at h = 1e-20 over the post-multiplicative camera
increment T Exp(d) and the additive point increment, rounded once to float64. Never from the analytic Jacobians, never from
the series of the kernel."""
import mpmath as mp

import geometry_ref as gr
from geometry_ref import F, V, precise

ABC_DPS = 150    # a, b, c at |s|, theta ~ 1e-13 cancel ~ 80 digits in the closed forms: evaluated at 150, handed back at 50


def abc(s, th):
    """a, b, c of V = a I + b [w]x + c [w]x^2 from the closed forms; s = 0 and th = 0 by their limits"""
    with mp.workdps(ABC_DPS):
        s, th = +s, +th
        E = mp.exp(s)
        a = (E - 1) / s if s != 0 else mp.mpf(1)
        if s == 0 and th == 0:
            b, c = mp.mpf(1) / 2, mp.mpf(1) / 6
        elif th == 0:
            b = (s * E - E + 1) / (s * s)
            c = (E * (s * s - 2 * s + 2) - 2) / (2 * s ** 3)
        elif s == 0:
            b = (1 - mp.cos(th)) / (th * th)
            c = (th - mp.sin(th)) / th ** 3
        else:
            u, v, w = E * mp.sin(th), E * mp.cos(th), 1 / (s * s + th * th)
            b = (u * s + (1 - v) * th) * w / th
            c = (a - ((v - 1) * s + u * th) * w) / (th * th)
        a, b, c = +a, +b, +c
    return +a, +b, +c


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def sim3_exp(v):
    """(R, tau, sigma) of Exp(v), v = [t | w | s]"""
    t, w, s = list(v[:3]), list(v[3:6]), v[6]
    a, b, c = abc(s, gr.norm(w))
    wt = cross(w, t)
    wwt = cross(w, wt)
    return gr.so3_exp(w), [a * t[i] + b * wt[i] + c * wwt[i] for i in range(3)], mp.exp(s)


def sim3_mul(T1, T2):
    """(R1, tau1, s1)(R2, tau2, s2) = (R1 R2, tau1 + s1 R1 tau2, s1 s2)"""
    R1, t1, s1 = T1
    R2, t2, s2 = T2
    return gr.matmul(R1, R2), [a + s1 * b for a, b in zip(t1, gr.matvec(R1, t2))], s1 * s2


def sim3_log(T):
    """the inverse of sim3_exp; the rotation's logarithm is the w >= 0 representative (the callers keep it away from pi)"""
    R, tau, sigma = T
    w = gr.so3_log(R)
    s = mp.log(sigma)
    a, b, c = abc(s, gr.norm(w))
    K = gr.hat(w)
    K2 = gr.matmul(K, K)
    Vm = mp.matrix([[a * int(i == j) + b * K[i][j] + c * K2[i][j] for j in range(3)] for i in range(3)])
    t = mp.lu_solve(Vm, mp.matrix(tau))
    return [t[0], t[1], t[2]] + list(w) + [s]


def project(T, intr, X):
    """Project_P2C_XYZ: x = T^-1 X, p - c = (fx x0/x2, fy x1/x2), k = intr[4] / (0.5 fx fy), uv = c + (1 + |p - c|^2 k)(p - c)"""
    R, tau, sigma = T
    x = [y / sigma for y in gr.matvec(gr.tr(R), [a - b for a, b in zip(X, tau)])]
    fx, fy, cx, cy, d = intr[:5]
    k = d / (fx * fy / 2)
    d0, d1 = fx * x[0] / x[2], fy * x[1] / x[2]
    g = 1 + (d0 * d0 + d1 * d1) * k
    return [cx + g * d0, cy + g * d1], x, (d0 * d0 + d1 * d1) * k


def cell(x):
    """class of |s| or of |w| against the reference's threshold: 0 zero, 1 in (0, 1e-12), 2 below 1e-6, 3 from 1e-6 on"""
    x = abs(x)
    return 0 if x == 0 else 1 if x < mp.mpf("1e-12") else 2 if x < mp.mpf("1e-6") else 3


@precise
def sim3_edge(cam, intr, X, z):
    """J0 (14: 2 x 7 column-major), J1 (6), r (2) of CEdgeP2C_XYZ_Sim3_G, camera first; aux: the camera-frame point (3),
    r^2 k; the branch row: class of |s|, class of |w| (4: beyond pi), kappa = 0, on the axis, behind the camera"""
    cam, intr, X, z = V(cam), V(intr), V(X), V(z)
    T = sim3_exp(cam)
    uv, x, r2k = project(T, intr, X)
    J0 = gr.cdiff(lambda d: project(sim3_mul(T, sim3_exp(d)), intr, X)[0], 7)
    J1 = gr.cdiff(lambda d: project(T, intr, [a + b for a, b in zip(X, d)])[0], 3)
    th = gr.norm(cam[3:6])
    br = [cell(cam[6]), 4 if th > mp.pi else cell(th), int(intr[4] == 0), int(x[0] == 0 and x[1] == 0), int(x[2] < 0)]
    return F(J0), F(J1), F([a - b for a, b in zip(z, uv)]), F(x + [r2k]), br


@precise
def sim3_plus(cam, d):
    """Log(Exp(cam) Exp(d)): the new camera (7), its rotation matrix (9, row-major), aux: the composite angle and s"""
    cam, d = V(cam), V(d)
    T = sim3_mul(sim3_exp(cam), sim3_exp(d))
    out = sim3_log(T)
    return F(out), F([T[0][i][j] for i in range(3) for j in range(3)]), F([gr.norm(out[3:6]), out[6]])


@precise
def exp_parts(v):
    """tau (3) and e^s of Exp(v), for the checks of a, b, c alone"""
    _, tau, sigma = sim3_exp(V(v))
    return F(tau + [sigma])
