"""The ternary edge CEdgeP2CI3D at 50 digits (mpmath, host only), on top of tests/geometry_ref.py: the model is
CBAJacobians::Project_P2C (geometry_ref.project_p2c_R, written from the model's definition), all three Jacobians are central
differences at h = 1e-20 over the documented increments -- the camera's Relative_to_Absolute, the point's sum, the plain sum
of Relative_to_Absolute_Intrinsics on fx fy cx cy kappa --, rounded once to float64. Also CVertexIntrinsics::Operator_Plus as
the reference writes it."""
import mpmath as mp

import geometry_ref as gr
from geometry_ref import F, V, precise

BAI_BR = gr.BA_BR


@precise
def bai_edge(cam, intr, X, z):
    """J0 (12), J1 (6), J2 (10: the five live columns, column-major), r (2) of CEdgeP2CI3D; aux: the camera-frame point (3),
    r2 k'; the branch row (BAI_BR: angle cell, kappa = 0, on the axis, behind the camera)"""
    cam, intr, X, z = V(cam), V(intr), V(X), V(z)
    t, R = gr.pose_R(cam)
    uv = gr.project_p2c_R(t, R, intr, X)
    J0 = gr.cdiff(lambda d: gr.project_p2c_R(*gr.rel_to_abs_R(t, R, d), intr, X), 6)
    J1 = gr.cdiff(lambda d: gr.project_p2c_R(t, R, intr, [a + b for a, b in zip(X, d)]), 3)
    J2 = gr.cdiff(lambda d: gr.project_p2c_R(t, R, [a + b for a, b in zip(intr, d)], X), 5)
    x = [a + b for a, b in zip(gr.matvec(R, X), t)]
    d0, d1 = intr[0] * x[0] / x[2], intr[1] * x[1] / x[2]
    r2k = (d0 * d0 + d1 * d1) * intr[4] / ((intr[0] + intr[1]) / 2)
    br = [gr.angle_cell(gr.norm(cam[3:])), int(intr[4] == 0), int(d0 == 0 and d1 == 0), int(x[2] < 0)]
    return F(J0), F(J1), F(J2), F([a - b for a, b in zip(z, uv)]), F(x + [r2k]), br


@precise
def intrinsics_plus(v, d):
    """CVertexIntrinsics::Operator_Plus as written: kappa through 0.5 fx fy of the old and of the new state"""
    v, d = V(v), V(d)
    den = (v[0] * v[1]) / 2
    dn = v[4] / den + d[4] / den
    out = [v[i] + d[i] for i in range(4)]
    return F(out + [dn * (out[0] * out[1]) / 2])
