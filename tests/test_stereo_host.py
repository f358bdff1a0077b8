"""Host side of stereo bundle adjustment (CVertexSCam + CVertexXYZ joined by CEdgeP2SC3D): the float64 mirror of
CBAJacobians::Project_P2SC and its analytic Jacobians (formats.stereo_expectation / stereo_linearize), the text tokens
(formats.load_stereo_graph / save_stereo_graph), the synthetic fixtures and the golden of the reference application
(tests/golden/stereo_lm.npz, tools/make_golden_stereo.py). No GPU."""
import os

import numpy as np

from slam_plus_plus_amd import formats, nonlinear, synth
from test_slam3d_host import dense_lambda

GOLD = os.path.join(os.path.dirname(__file__), "golden", "stereo_lm.npz")


def edge_case_state(p):
    """the fixture's states with the cases the projection's geometry has branches or degeneracies for. Returns (cams,
    intr, points, cases): cases["small"]: an observation whose camera has ||axis-angle|| < 1e-10 (small-angle branch);
    ["pi"]: one whose camera's angle is within 1e-3 of pi; ["axis"]: one whose point lies exactly on the optical axis of
    its (left) camera, rho = 0 -- that camera is put at [0 0 10 | 0 0 0] (R = I exactly, in every implementation) with a
    non-zero d, the point at (0, 0, -3); ["axis_right"]: another observation of that camera, its point at (b, 0, -3): on the
    RIGHT camera's axis, rho_right = 0; ["d0"]: an observation whose camera has d = 0."""
    g = p.geometry
    cams, intr, pts = g["cams"].copy(), g["intr"].copy(), g["points"].copy()
    co, po = g["cam_of"], g["pt_of"]
    k0 = int(np.flatnonzero(intr[co, 4] == 0)[0])
    k1 = int(np.flatnonzero((co != co[k0]) & (po != po[k0]))[0])
    free = (co != co[k0]) & (co != co[k1]) & (po != po[k0]) & (po != po[k1])
    k2 = int(np.flatnonzero(free & (intr[co, 4] != 0))[0])
    k3 = int(np.flatnonzero(free & (co == co[k2]) & (po != po[k2]))[0])
    cams[co[k0], 3:] = 1e-11 * np.array([0.6, -0.8, 0.0])
    cams[co[k0], :3] = [0.1, -0.2, 10.0]
    cams[co[k1], 3:] = (np.pi - 5e-4) * np.array([2.0, -1.0, 2.0]) / 3.0
    cams[co[k1], :3] = [0.0, 0.0, 10.0]
    cams[co[k2]] = [0.0, 0.0, 10.0, 0.0, 0.0, 0.0]
    pts[po[k2]] = [0.0, 0.0, -3.0]
    pts[po[k3]] = [intr[co[k3], 5], 0.0, -3.0]
    return cams, intr, pts, dict(small=k0, pi=k1, axis=k2, axis_right=k3, d0=k0)


def test_jacobians_against_central_differences():
    """J0 / J1 of the (6, 3, 3) group against central difference quotients of the mirror's own expectation (written as
    the reference writes it: the point moved by -b (row 0 of R)^T and rotated again) under the reference's (+): camera
    (+) d = Relative_to_Absolute (formats.se3_plus), point + d. So the check also covers the x - b e0 form the Jacobians
    are derived in. Expectations are pixel-sized, |e| up to ~700, and so are their third derivatives w.r.t. a rotation:
    round-off eps |e| / h and truncation h^2 |e(3)| / 6 balance at h = (3 eps)^(1/3) ~ 1e-5, where each is ~1e-8 px -- 1e-10
    of the largest Jacobian entry (~2e2). The bound is 1e-8 relative, two orders over that: the check guards formulas,
    not digits. Measured: see DESIGN section 16.
    At rho = 0 the expectation c + (1 + k |q|) q is differentiable, with the Jacobian of q itself, but its second
    derivative jumps: along a direction in which q moves at the rate a, the central quotient is off by k |a| a h.
    The two observations on an optical axis get that allowance, with |a|^2 <= 2 S^2, S the block's largest entry:
    2 k h S^2. That alone would pin the on-axis Jacobian to ~1e-4 px only, so the limit is checked as well: with d = 0
    the expectation is c + q, smooth on the axis, so its quotient gets the plain 1e-8 bound there; and the analytic
    Jacobian with d != 0 at rho = 0 is that of q, (1 + 0 k) I + k q 0^T = I in front of it -- equal to the d = 0 one
    bit for bit, in the rows whose rho is 0 (an observation on the left axis has rho_right != 0, and the other way
    round)."""
    p = synth.make("stereo_interleaved")
    cams, intr, pts, cases = edge_case_state(p)
    obs = p.geometry["obs"]
    co, po = p.geometry["cam_of"], p.geometry["pt_of"]
    cam, itr, X = cams[co], intr[co], pts[po]
    ang = np.linalg.norm(cam[:, 3:], axis=1)
    assert 0 < ang[cases["small"]] < 1e-10 and abs(ang[cases["pi"]] - np.pi) < 1e-3 and itr[cases["d0"], 4] == 0
    e = formats.stereo_expectation(cam, itr, X)
    c = itr[:, 2:4]
    assert np.array_equal(e[cases["axis"], :2], c[cases["axis"]]) and itr[cases["axis"], 4] != 0      # rho = 0 exactly
    assert e[cases["axis_right"], 2] == c[cases["axis_right"], 0]                                       # rho_right = 0
    g = formats.stereo_linearize(cams, intr, pts, obs, p.geometry["cam_id"], p.geometry["pt_id"], p.geometry["info"])
    k, h = co.size, 1e-5
    J0 = g.J0.reshape(k, 6, 3).transpose(0, 2, 1)
    J1 = g.J1.reshape(k, 3, 3).transpose(0, 2, 1)
    assert np.isfinite(J0).all() and np.isfinite(J1).all()
    assert np.array_equal(g.r, obs[:, 2:5] - e) and (g.d0, g.d1, g.rd) == (6, 3, 3) and g.Om.shape == (k, 9)
    num0, num1 = np.empty_like(J0), np.empty_like(J1)
    for col in range(6):
        d = np.zeros((k, 6))
        d[:, col] = h
        num0[:, :, col] = (formats.stereo_expectation(formats.se3_plus(cam, d), itr, X) -
                           formats.stereo_expectation(formats.se3_plus(cam, -d), itr, X)) / (2 * h)
    for col in range(3):
        d = np.zeros((k, 3))
        d[:, col] = h
        num1[:, :, col] = (formats.stereo_expectation(cam, itr, X + d) - formats.stereo_expectation(cam, itr, X - d)) / (2 * h)
    kink = [cases["axis"], cases["axis_right"]]
    smooth = np.setdiff1d(np.arange(k), kink)
    for name, num, J in (("J0", num0, J0), ("J1", num1, J1)):
        err = np.abs(num - J)[smooth].max() / np.abs(J).max()
        print(name, "difference quotient vs analytic, relative max-abs: %.3e (largest entry %.3e)" % (err, np.abs(J).max()))
        assert err <= 1e-8, (name, err)
        for kc in (cases["small"], cases["pi"], cases["d0"]):   # the cases themselves, each relative to its own block
            assert np.abs(num[kc] - J[kc]).max() <= 1e-8 * max(1.0, np.abs(J[kc]).max()), (name, kc)
        for kc in kink:
            S = np.abs(J[kc]).max()
            allow = 2 * itr[kc, 4] / (0.5 * (itr[kc, 0] + itr[kc, 1])) * h * S * S
            print(name, "rho = 0, observation %d: %.3e px, allowance %.3e, largest entry %.3e" % (
                kc, np.abs(num[kc] - J[kc]).max(), allow, S))
            assert np.abs(num[kc] - J[kc]).max() <= 1e-8 * S + allow, (name, kc)
    # the limit itself: the same lens without distortion
    intr_q = intr.copy()
    intr_q[co[kink], 4] = 0.0
    itr_q = intr_q[co]
    gq = formats.stereo_linearize(cams, intr_q, pts, obs, p.geometry["cam_id"], p.geometry["pt_id"], p.geometry["info"])
    Jq0 = gq.J0.reshape(k, 6, 3).transpose(0, 2, 1)
    Jq1 = gq.J1.reshape(k, 3, 3).transpose(0, 2, 1)
    for kc, rows in ((cases["axis"], [0, 1]), (cases["axis_right"], [2])):
        assert np.array_equal(J0[kc][rows], Jq0[kc][rows]) and np.array_equal(J1[kc][rows], Jq1[kc][rows]), kc
        c6, x3 = cam[kc:kc + 1], X[kc:kc + 1]
        for Jq, n, plus in ((Jq0[kc], 6, lambda d: (formats.se3_plus(c6, d), x3)), (Jq1[kc], 3, lambda d: (c6, x3 + d))):
            S = np.abs(Jq).max()
            for col in range(n):
                d = np.zeros((1, n))
                d[0, col] = h
                quot = (formats.stereo_expectation(plus(d)[0], itr_q[kc:kc + 1], plus(d)[1]) -
                        formats.stereo_expectation(plus(-d)[0], itr_q[kc:kc + 1], plus(-d)[1]))[0] / (2 * h)
                err = np.abs(quot - Jq[:, col]).max()
                assert err <= 1e-8 * S, (kc, n, col, err)
            print("rho = 0, observation %d, d = 0 (the limit), %d columns: within 1e-8 of the largest entry %.3e" % (kc, n, S))


def test_round_trip(tmp_path):
    """save -> load: points, measurements and information come back bit for bit (%.17g), the cameras through centre +
    quaternion and back. Measured: 3.6e-15 (stereo_small), 5.3e-15 (stereo_interleaved) on entries of up to 10; the bound
    is the one tests/test_formats.py gives VERTEX_CAM, 1e-12. d comes back through d / f * f: 2 ulp at the most."""
    for name in ("stereo_small", "stereo_interleaved"):
        g = synth.make(name).geometry
        path = str(tmp_path / (name + ".txt"))
        formats.save_stereo_graph(path, g["cams"], g["intr"], g["points"], g["obs"], g["info"], g["cam_id"], g["pt_id"])
        q = formats.load_stereo_graph(path)
        oc, op = np.argsort(g["cam_id"]), np.argsort(g["pt_id"])      # the file lists the vertices in id order
        assert np.array_equal(q["cam_id"], g["cam_id"][oc]) and np.array_equal(q["pt_id"], g["pt_id"][op])
        assert np.array_equal(q["points"], g["points"][op])
        err = np.abs(q["cams"] - g["cams"][oc]).max()
        print(name, "cameras after the quaternion round trip: %.3e" % err)
        assert err < 1e-12
        assert np.array_equal(q["intr"][:, [0, 1, 2, 3, 5]], g["intr"][oc][:, [0, 1, 2, 3, 5]])
        assert np.abs(q["intr"][:, 4] - g["intr"][oc, 4]).max() <= 2 * np.finfo(float).eps * g["intr"][:, 4].max()
        # edges in the order given; camera / point INDICES refer to the file's vertex order
        assert np.array_equal(q["cam_id"][q["obs"][:, 0].astype(int)], g["cam_id"][g["cam_of"]])
        assert np.array_equal(q["pt_id"][q["obs"][:, 1].astype(int)], g["pt_id"][g["pt_of"]])
        assert np.array_equal(q["obs"][:, 2:], g["obs"][:, 2:]) and np.array_equal(q["info"], g["info"])
        # EDGE_P2SC is an alias; problem_from_graph hands the file over as ONE (6, 3, 3) group
        with open(path) as f:
            text = f.read()
        with open(path, "w") as f:
            f.write(text.replace("EDGE_PROJECT_P2SC", "EDGE_P2SC"))
        q2 = formats.load_stereo_graph(path)
        assert all(np.array_equal(q[k], q2[k]) for k in q)
        prob, what = formats.problem_from_graph(path)
        ref = synth.make(name)
        assert (prob.d0, prob.d1, prob.rd) == (6, 3, 3) and "stereo BA" in what and np.array_equal(prob.dim, ref.dim)
        assert np.array_equal(prob.v0, ref.v0) and np.array_equal(prob.v1, ref.v1) and np.array_equal(prob.Om, ref.Om)
        assert np.abs(prob.r - ref.r).max() < 1e-9


def test_fixtures_are_what_the_issue_describes():
    for name, (nc, npts) in (("stereo_small", (6, 40)), ("stereo_interleaved", (30, 150))):
        p = synth.make(name)
        g = p.geometry
        assert (p.dim == 6).sum() == nc and (p.dim == 3).sum() == npts and (p.d0, p.d1, p.rd) == (6, 3, 3)
        per_pt, per_cam = np.bincount(g["pt_of"], minlength=npts), np.bincount(g["cam_of"], minlength=nc)
        assert len(set(zip(g["cam_of"].tolist(), g["pt_of"].tolist()))) == g["cam_of"].size       # no pair twice
        assert (g["intr"][:, 4] != 0).sum() == nc // 2
        depth = np.linalg.norm(g["truth"]["cams"][:, :3], axis=1)                                   # |t| = |C|: the scene is at the origin
        assert np.allclose(g["intr"][:, 5] / depth, 1 / 20, rtol=0.05)
        if name == "stereo_small":
            assert per_pt.min() >= 2 and per_pt.max() <= 6 and np.array_equal(g["cam_id"], np.arange(nc))
        else:   # one point seen by every camera, one camera beyond the sequential kernel's 24 entries, shuffled ids
            assert per_pt.max() == nc and (per_pt == nc).sum() == 1 and per_pt.min() >= 2 and per_cam.max() > 24
            assert 0.35 < (p.v1 < p.v0).mean() < 0.65
        s = synth.stereo_states(p)
        e = formats.stereo_expectation(s["cams"][s["cam_of"]], s["intr"][s["cam_of"]], s["points"][s["pt_of"]])
        assert np.abs(s["meas"] - (e + p.r)).max() < 1e-12                                          # measurements = expectation + r
        base = formats.slam3d_offsets(p.dim)
        assert np.array_equal(s["cam_dxoff"], base[g["cam_id"]]) and np.array_equal(s["pt_dxoff"], base[g["pt_id"]])


class HostStereoPath:
    """the LM path on the host: numpy linearization (the mirror), dense float64 Lambda and solve"""

    def begin(self, s):
        self.s = s
        self.trace = []     # True per accepted step, False per rejected one

    def linearize(self):
        self.prob = self.s.linearize()

    def max_hessian_diag(self):
        p = self.prob
        Om = p.Om.reshape(-1, 3, 3)
        return max(np.einsum("eci,eij,ecj->ec", J.reshape(-1, d, 3), Om, J.reshape(-1, d, 3)).max()
                   for J, d in ((p.J0, 6), (p.J1, 3)))

    def chi2(self):
        self.linearize()
        return float(np.einsum("ei,eij,ej->", self.prob.r, self.prob.Om.reshape(-1, 3, 3), self.prob.r))

    def solve(self, alpha):
        L, eta = dense_lambda([self.prob])
        L[np.diag_indices_from(L)] += alpha
        self.dx, self.eta = np.linalg.solve(L, eta), eta
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


def test_lm_on_the_host_converges_on_both_fixtures():
    for name in ("stereo_small", "stereo_interleaved"):
        s = nonlinear.CStereoBundleAdjustment.from_problem(synth.make(name))
        x0 = s.state()
        s.plus(np.zeros(int(synth.make(name).dim.sum())))
        assert all(np.abs(a - b).max() < 1e-14 * 10 for a, b in zip(s.state(), x0))
        solver = nonlinear.CNonlinearSolver_Lambda_LM(s, path=HostStereoPath())
        solver.Optimize(10, 1e-4)
        h = solver.chi2_history
        assert all(b <= a for a, b in zip(h, h[1:])) and h[-1] < 0.05 * h[0], (name, h)


def _golden_system(tmp_path):
    gold = np.load(GOLD)
    path = str(tmp_path / "g.txt")
    with open(path, "w") as f:
        f.write("\n".join(gold["lines"].tolist()) + "\n")
    return gold, formats.load_stereo_graph(path)


def _states_of(gold, key, g):
    """initial.txt / solution.txt: one vertex per line in id order, 6 numbers for a camera and 3 for a point"""
    base = formats.slam3d_offsets(gold["dim"])
    x = gold[key]
    return x[base[g["cam_id"]][:, None] + np.arange(6)], x[base[g["pt_id"]][:, None] + np.arange(3)]


def test_loader_matches_the_reference_application(tmp_path):
    """tests/golden/stereo_lm.npz: the reference application (SolveBAStereoImpl.cpp) on the stereo_small fixture written by
    save_stereo_graph. Its initial.txt -- the parser's inversion of the camera-to-world pose, six decimals -- pins
    load_stereo_graph; the initial chi2 it prints with two decimals (16825.55) pins the expectation, the residual, the
    information and the parser's scaling of d (the file's d times 0.5 (fx + fy))."""
    gold, g = _golden_system(tmp_path)
    dim = np.empty(gold["dim"].size, dtype=np.int32)
    dim[g["cam_id"]], dim[g["pt_id"]] = 6, 3
    assert np.array_equal(dim, gold["dim"])
    cams, pts = _states_of(gold, "init", g)
    assert np.abs(g["cams"] - cams).max() <= 5e-7 * max(1.0, np.abs(cams).max())
    assert np.abs(g["points"] - pts).max() <= 5e-7 * max(1.0, np.abs(pts).max())
    chi2 = nonlinear.CStereoBundleAdjustment.from_problem(g).chi2()
    print("initial chi2 %.6f, the application prints %.2f" % (chi2, float(gold["initial_chi2"])))
    assert abs(chi2 - float(gold["initial_chi2"])) <= 0.006


def test_lm_matches_the_reference_application_on_the_final_chi2(tmp_path):
    """CNonlinearSolver_Lambda_LM on CStereoBundleAdjustment, host path with a dense float64 solve, against the
    application's Optimize(5, 0.01) on the same file. The application converges: chi2 16825.55 -> 294.17 -> 292.89 and
    stops at its third solve (||dx|| 0.0036 < 0.01), every step accepted. It differentiates with forward differences
    (delta = 1e-9), this code analytically, so only the final chi2 is compared: chi2 of the mirror at the final states of
    this loop against chi2 of the mirror at the application's solution.txt (six decimals; it prints 292.89).
    Measured: 292.893632367 here, 292.893634529 for solution.txt, relative difference 7.38e-9; the bound is 4 x that, the
    factor tests/parity.py grants: 3.0e-8. This loop, too, takes three solves and accepts both steps."""
    gold, g = _golden_system(tmp_path)
    s = nonlinear.CStereoBundleAdjustment.from_problem(g)
    solver = nonlinear.CNonlinearSolver_Lambda_LM(s, path=HostStereoPath())
    solver.Optimize(int(gold["max_iter"]), float(gold["threshold"]))
    cams, pts = _states_of(gold, "final", g)
    ref = nonlinear.CStereoBundleAdjustment(cams, g["intr"], pts, g["obs"], g["info"], g["cam_id"], g["pt_id"])
    d = abs(s.chi2() - ref.chi2()) / ref.chi2()
    print("final chi2 %.9f here, %.9f at solution.txt (printed %.2f), relative difference %.3e, iterations %d, accepted %s" % (
        s.chi2(), ref.chi2(), float(gold["final_chi2"]), d, solver.n_iterations, solver.path.trace))
    assert abs(ref.chi2() - float(gold["final_chi2"])) <= 0.006
    assert d <= 3.0e-8
