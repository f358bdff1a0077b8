"""Host side of self-calibrating bundle adjustment (CVertexCam + CVertexXYZ + CVertexIntrinsics joined by the ternary
CEdgeP2CI3D): the float64 mirror (formats.bai_expectation / bai_linearize / bai_intrinsics_plus) against the 50-digit
reference of tests/bai_ref.py, the text tokens, the synthetic fixtures, the Levenberg-Marquardt loop on the host, the golden
of the reference application (tests/golden/bai_lm.npz, tools/make_golden_bai.py) and the Schur plan of the padded
structure. No GPU."""
import os
import re

import numpy as np
import pytest

from slam_plus_plus_amd import api, formats, nonlinear
from slam_plus_plus_amd.blockcsc import structure_from_pairs
import bai_cases as bc
import bai_ref
import geometry_cases as gc

GOLD = os.path.join(os.path.dirname(__file__), "golden", "bai_lm.npz")
EDGES = os.path.join(os.path.dirname(__file__), "golden", "bai_edges.npz")


def quotients(got, want, scale):
    """|got - want| / (eps scale), entry by entry; where the scale is 0 the entries must be equal (quotient 0, else inf)"""
    err, sc = np.abs(got - want), bc.EPS * scale
    return np.where(sc > 0, err / np.where(sc > 0, sc, 1.0), np.where(err > 0, np.inf, 0.0))


def test_mirror_against_the_50_digit_reference_and_the_constant_is_the_rule():
    """the reference is recomputed here (mpmath) and must be what tests/golden/bai_edges.npz holds; the mirror meets
    |mirror - reference| <= C eps scale, and C is 8 x the largest quotient, at least 8, rounded up to a power of two"""
    cams, intr, pts, obs = bc.edge_cases()
    g = np.load(EDGES)
    for k, a in (("cams", cams), ("intr", intr), ("pts", pts), ("obs", obs)):
        assert np.array_equal(g[k], a), k
    ref = [bai_ref.bai_edge(cams[int(o[0])], intr[int(o[2])], pts[int(o[1])], o[3:5]) for o in obs]
    J2 = np.zeros((obs.shape[0], 12))
    J2[:, :10] = np.array([o[2] for o in ref])
    want = {"J0": np.array([o[0] for o in ref]), "J1": np.array([o[1] for o in ref]), "J2": J2, "r": np.array([o[3] for o in ref])}
    for k in want:
        assert np.array_equal(want[k], g[k]), k
    br = np.array([o[5] for o in ref])
    # the cases: every cell of the camera's angle (0, below 1e-12, the series' side and the other side of 1e-6, generic,
    # beyond pi, beyond 2 pi), kappa = 0, on the axis, behind the camera; fx != fy; |X| = 1e3; r2 k = 0.3
    assert set(br[:, 0]) >= {0, 2, 5, 6} and br[:, 1].any() and br[:, 2].any() and br[:, 3].any()
    assert (intr[:, 0] != intr[:, 1]).all() and np.abs(pts).max() >= 1e3 and np.abs(g["aux"][:, 3] - 0.3).min() < 0.01
    io, co = obs[:, 2].astype(int), obs[:, 0].astype(int)
    assert (io > co).any() and (io < co).any() and np.bincount(io).max() >= 3       # ids reversed and repeated
    p = formats.bai_linearize(cams, intr, pts, obs)
    assert np.isfinite(p.J0).all() and np.isfinite(p.J2).all() and not p.J2[:, 10:].any()
    on_axis = int(np.flatnonzero(br[:, 2])[0])
    assert np.isfinite(p.J2[on_axis]).all() and not p.J2[on_axis, [0, 1, 2, 3, 8, 9]].any()
    s = bc.edge_scales(cams, intr, pts, obs, g["aux"])
    for k, got in (("J0", p.J0), ("J1", p.J1), ("J2", p.J2), ("r", p.r)):
        q = quotients(got, want[k], s[k]).max()
        print(k, "largest mirror quotient %.3f -> C %d" % (q, gc.c_rule(q)))
        assert q <= bc.C[k] and bc.C[k] == gc.c_rule(q), (k, q)
    for v, d, out in zip(g["upd_v"], g["upd_d"], g["upd_out"]):
        assert np.array_equal(bai_ref.intrinsics_plus(v, d), out)
        got = formats.bai_intrinsics_plus(v[None], d[None])[0]
        assert np.all(np.abs(got - out) <= 4 * bc.EPS * np.abs(out)), (got, out)
    assert np.array_equal(formats.bai_intrinsics_plus(g["upd_v"][3:], g["upd_d"][3:])[0, :4], g["upd_v"][3, :4])


def test_the_expectation_is_the_residual_of_the_mirror():
    p = bc.fixture("bai_small")
    g = p.geometry
    e = formats.bai_expectation(g["cams"][g["cam_of"]], g["intr"][g["intr_of"]], g["points"][g["pt_of"]])
    assert np.abs(p.r - (g["obs"][:, 3:5] - e)).max() <= 1e-10
    assert (p.d0, p.d1, p.d2, p.live2, p.rd) == (6, 3, 6, 5, 2) and p.J2.shape == (p.v0.size, 12)
    pts_seen = {(int(a), int(b)) for a, b in zip(g["pt_of"], g["intr_of"])}
    assert any((j, 0) in pts_seen and (j, 1) in pts_seen for j in range(40))   # a point with two (point, intrinsics) blocks


def _flat(s):
    """the states in vertex id order, as initial.txt / solution.txt list them"""
    rows = {}
    for ids, vals in ((s.intr_id, s.intr), (s.cam_id, s.cams), (s.pt_id, s.points)):
        for i, v in zip(ids, vals):
            rows[int(i)] = v
    return np.concatenate([rows[k] for k in sorted(rows)])


def _golden_system(tmp_path):
    gold = np.load(GOLD)
    path = str(tmp_path / "g.txt")
    with open(path, "w") as f:
        f.write("\n".join(gold["lines"].tolist()) + "\n")
    return gold, nonlinear.CBundleAdjustmentIntrinsics.from_problem(formats.load_bai_graph(path))


def test_round_trip_and_loader(tmp_path):
    """save -> load to 1e-12; the golden's lines are what the fixture writes; the loader reproduces the application's
    initial states (6 decimals printed) and its initial chi2 (6 decimals printed)"""
    for name in ("bai_small", "bai_tiny"):
        for layout in ("first", "interleaved"):
            g = bc.fixture(name, layout).geometry
            path = str(tmp_path / "rt.txt")
            formats.save_bai_graph(path, g["cams"], g["intr"], g["points"], g["obs"], g["info"], g["cam_id"], g["pt_id"], g["intr_id"])
            L = formats.load_bai_graph(path)
            a = nonlinear.CBundleAdjustmentIntrinsics.from_problem(g)
            b = nonlinear.CBundleAdjustmentIntrinsics.from_problem(L)
            fa, fb = _flat(a), _flat(b)
            assert np.all(np.abs(fa - fb) <= 1e-12 * np.maximum(1.0, np.abs(fa)))
            assert abs(a.chi2() - b.chi2()) <= 1e-9 * a.chi2()
            # the file lists the vertices in id order: observation columns come back as indices into that order
            assert np.array_equal(np.sort(L["cam_id"]), L["cam_id"]) and L["obs"].shape == g["obs"].shape
    gold, s = _golden_system(tmp_path)
    g = bc.fixture("bai_small").geometry
    assert gold["lines"].tolist() == formats.bai_lines(g["cams"], g["intr"], g["points"], g["obs"], g["info"], g["cam_id"],
                                                      g["pt_id"], g["intr_id"])
    assert np.array_equal(gold["dim"], np.array([5] * 2 + [6] * 6 + [3] * 40))
    assert np.abs(_flat(s) - gold["init"]).max() <= 0.5e-6 + 1e-12
    first = float(re.search(r"initial chi2: ([-+0-9.eE]+)", "\n".join(gold["output"].tolist())).group(1))
    assert abs(s.chi2() - first) <= 0.5e-6 + 1e-9 and abs(first - float(gold["initial_chi2"])) <= 0.5e-2


@pytest.mark.parametrize("name", bc.FIXTURES)
def test_lm_on_the_host_converges(name):
    """monotone, below 0.05 of the initial chi2 within 5 iterations; a zero increment leaves the state alone"""
    s = nonlinear.CBundleAdjustmentIntrinsics.from_problem(bc.fixture(name))
    x0 = s.state()
    s.plus(np.zeros(int(bc.fixture(name).dim.sum())))
    assert all(np.abs(a - b).max() <= 1e-13 * max(1.0, np.abs(b).max()) for a, b in zip(s.state(), x0))
    s, solver = bc.host_lm(name)
    h = solver.chi2_history
    print(name, ["%.6g" % c for c in h])
    assert solver.n_iterations == 5 and len(h) == 6
    assert all(b < a for a, b in zip(h, h[1:])) and h[-1] < 0.05 * h[0], (name, h)


def test_host_lm_against_the_application(tmp_path):
    """The application differentiates all three Jacobians with forward differences of delta = 1e-9, fx ~ 500 included, so
    its steps differ from the analytic ones by the noise of that and the difference grows over the 5 iterations. Measured
    here on the CPU: the final states differ from solution.txt by 8.6e-6 max(1, |x|) at most, the final
    chi2 (218.663788 printed) by 1.37e-2. The bounds are 4 x that, never below what the files print (6 decimals)."""
    gold, s = _golden_system(tmp_path)
    solver = nonlinear.CNonlinearSolver_Lambda_LM(s, path=bc.HostBAIPath())
    solver.Optimize(int(gold["max_iter"]), float(gold["threshold"]))
    out = "\n".join(gold["output"].tolist())
    chi = [float(x) for x in re.findall(r"^chi2: ([-+0-9.eE]+)", out, flags=re.M)]
    assert solver.n_iterations == 5 and len(chi) == 5 and "solver took 5 iterations" in out
    d = np.abs(_flat(s) - gold["final"]) / np.maximum(1.0, np.abs(gold["final"]))
    print("states: %.3e max(1, |x|); chi2 %.6f against %.6f: %.3e" % (d.max(), solver.chi2_history[-1], chi[-1],
                                                                     abs(solver.chi2_history[-1] - chi[-1])))
    assert d.max() <= max(4 * 8.6e-6, 0.5e-6)
    assert abs(solver.chi2_history[-1] - chi[-1]) <= max(4 * 1.37e-2, 0.5e-6)
    assert abs(chi[-1] - float(gold["final_chi2"])) <= 0.5e-2


@pytest.mark.parametrize("name", bc.FIXTURES)
def test_padded_schur_plan(name):
    """the padded structure -- the intrinsics a 6-wide vertex joined to its cameras and points -- is accepted by the Schur
    plan with poses = cameras + intrinsics; on bai_hub the hub's block of S is split into items"""
    p = bc.fixture(name)
    v = [np.asarray(a, dtype=np.int64) for a in (p.v0, p.v1, p.v2)]
    rows = np.concatenate([np.minimum(v[a], v[b]) for a, b in ((0, 1), (0, 2), (1, 2))])
    cols = np.concatenate([np.maximum(v[a], v[b]) for a, b in ((0, 1), (0, 2), (1, 2))])
    lam, _, _ = structure_from_pairs(p.dim, rows, cols)
    plan = api.schur_plan_host(lam)
    print(name, plan)
    assert plan["nc"] == p.nc + p.ni and plan["nl"] == p.npts
    assert plan["no"] == np.unique(v[0] * p.dim.size + v[1]).size + np.unique(v[2] * p.dim.size + v[1]).size
    if name == "bai_hub":
        assert plan["n_multi"] >= 1
    order, _, _, _ = api.schur_cam_order_host(lam)
    assert np.array_equal(np.sort(order), np.arange(p.nc + p.ni))
