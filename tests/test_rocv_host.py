"""Host side of range-only constant-velocity SLAM (ROCV): the numpy mirror of the two edge models against a 50-digit
reference (tests/rocv_ref.py), the text tokens (formats.load_rocv_graph / save_rocv_graph), the synthetic fixtures and
the golden of the reference application (tools/make_golden_rocv.py -> tests/golden/rocv_gn.npz). No GPU."""
import os

import numpy as np

import rocv_ref
from slam_plus_plus_amd import formats, nonlinear, synth

GOLD = os.path.join(os.path.dirname(__file__), "golden", "rocv_gn.npz")


def _mirror():
    p, l, z = rocv_ref.range_cases()
    x0, x1, dt = rocv_ref.cv_cases()
    J0, J1, r = formats.rocv_range_model(p[:, :3], l, z)
    A, B, rc = formats.rocv_cv_model(x0, x1, dt)
    return {"rng_J0": J0, "rng_J1": J1, "rng_r": r, "cv_J0": A, "cv_J1": B, "cv_r": rc}


def test_mirror_against_the_50_digit_reference():
    """|mirror - reference| <= C eps scale, C by DESIGN section 18's rule: 8 x the largest quotient, a quotient below 1
    counting as 1, rounded up to a power of two. Measured quotients: range J0 / J1 / r 0.5 / 0.5 / 0.83, constant velocity
    0 / 0 / 0.22 (the Jacobians' entries are exact), so C = 8 throughout."""
    q = rocv_ref.quotients(_mirror())
    print("mirror quotients:", {k: round(v, 3) for k, v in q.items()})
    for k, v in q.items():
        c = 8 * max(1.0, v)
        assert rocv_ref.C[k] == 2 ** int(np.ceil(np.log2(c))), (k, v)
        assert v <= rocv_ref.C[k]


def test_the_cases_are_what_the_issue_lists():
    p, l, z = rocv_ref.range_cases()
    e = np.linalg.norm(p[:, :3] - l, axis=1)
    assert e[1] == 0.0 and 0.5e-12 < e[2] < 2e-12 and abs(e[3] - 1e6) < 1.0
    assert ((p[:, :3] == l).sum(axis=1) == 2).sum() >= 2          # receiver and transmitter coincide in two coordinates
    x0, x1, dt = rocv_ref.cv_cases()
    assert (dt == 0).any() and (dt < 0).any()
    m, ref = _mirror(), rocv_ref.reference()
    assert not m["rng_J0"][1].any() and not m["rng_J1"][1].any() and m["rng_r"][1] == z[1]     # e = 0: zeros and r = z
    assert not ref["rng_J0"][1].any() and ref["rng_r"][1] == z[1]
    assert np.array_equal(m["cv_J1"], np.tile(np.eye(6), (dt.size, 1, 1)))
    # the reference's signs: J0 = -[I, dt I; 0, I], r = -(x1 - expectation)
    k = 0
    assert np.array_equal(m["cv_J0"][k], -(np.eye(6) + np.diag([dt[k]] * 3, 3)))
    assert np.allclose(m["cv_r"][k][3:], x0[k, 3:] - x1[k, 3:])
    # linearize() lays the same numbers out column-major, three groups, the last one unary
    state, (o0, o1, zz), (c0, c1, dd) = rocv_ref.cases_as_state()
    assert np.array_equal(state[o0[2]:o0[2] + 6], p[2]) and np.array_equal(state[c1[3]:c1[3] + 6], x1[3])


def test_round_trip(tmp_path):
    for name in ("rocv_small", "rocv_interleaved"):
        p = synth.make(name)
        path = str(tmp_path / (name + ".txt"))
        formats.save_rocv_graph(path, p.dim, p.state, p.cv, p.cv_info, p.rng, p.rng_info, p.pri, p.pri_info, p.cv_seq, p.rng_seq,
                                p.pri_seq, p.explicit)
        g = formats.load_rocv_graph(path)
        assert np.array_equal(g["dim"], p.dim) and np.array_equal(g["explicit"], p.explicit)
        for grp in ("cv", "rng", "pri"):     # the file lists the edges in the global order; %.17g: every double comes back
            o = np.argsort(p[grp + "_seq"])
            for k in (grp, grp + "_info", grp + "_seq"):
                assert np.array_equal(g[k], p[k][o]), k
        # receivers without a ROCV:RECEIVER line start where CConstVelocity_Initializer puts them: how the fixture starts them
        assert (~p.explicit).sum() >= 4 and np.array_equal(g["state"], p.state)
        groups, what = formats.problem_from_graph(path)
        assert [(q.d0, q.d1, q.rd) for q in groups] == [(6, 6, 6), (6, 3, 1), (3, 0, 3)] and "ROCV" in what
        assert groups[2].v1 is None and groups[2].J1.size == 0 and not groups[2].r.any() and groups[0].unary_vertex == -1


def test_parser_quirks(tmp_path):
    """a ROCV:DELTA_TIME line with i > j is dropped (ParsePrimitives.h:1638-1656); the six numbers of a _UF line are the
    information as given, symmetrised, never inverted (:1460-1471); RECEIVER_GTfake is ignored; a vertex an edge meets first
    is the null vertex, the second receiver of a constant-velocity edge starts at (p + v dt, v)"""
    path = str(tmp_path / "q.txt")
    om = " ".join(["1"] + ["0"] * 5 + ["2"] + ["0"] * 4 + ["3"] + ["0"] * 3 + ["4", "0", "0", "5", "0", "6"])
    with open(path, "w") as f:
        f.write("ROCV:RECEIVER 0 1 2 3 0.5 -1 2\nROCV:RECEIVER_GTfake 0 9 9 9 9 9 9\n"
                "ROCV:DELTA_TIME 0 1 2.0 %s\nROCV:DELTA_TIME 1 0 2.0 %s\n" % (om, om) +
                "ROCV:RANGE 1 2 7.5 400\nROCV:TRANSMITTER_UF 2 4 0.5 0.25 5 0.125 6\nrocv:range 0 2 3.5 100\n")
    g = formats.load_rocv_graph(path)
    assert list(g["dim"]) == [6, 6, 3] and g["cv"].shape[0] == 1 and g["rng"].shape[0] == 2
    assert np.array_equal(g["state"], [1, 2, 3, 0.5, -1, 2, 2.0, 0.0, 7.0, 0.5, -1, 2, 0, 0, 0])
    assert np.array_equal(g["pri_info"][0], [[4, 0.5, 0.25], [0.5, 5, 0.125], [0.25, 0.125, 6]])
    assert np.array_equal(np.diag(g["cv_info"][0]), [1, 2, 3, 4, 5, 6])
    assert list(g["cv_seq"]) == [0] and list(g["rng_seq"]) == [1, 3] and list(g["pri_seq"]) == [2]
    assert list(g["explicit"]) == [True, False, False]


def test_fixtures_are_what_the_issue_describes():
    for name, (nr, nt) in (("rocv_small", (40, 5)), ("rocv_interleaved", (150, 8))):
        p = synth.make(name)
        assert (p.dim == 6).sum() == nr and (p.dim == 3).sum() == nt and p.unary_vertex == -1
        assert p.cv.shape[0] == nr - 1 and (p.cv[:, 0] < p.cv[:, 1]).all() and p.pri.size == nt
        n_e = p.cv.shape[0] + p.rng.shape[0] + p.pri.size
        assert np.array_equal(np.sort(np.concatenate([p.cv_seq, p.rng_seq, p.pri_seq])), np.arange(n_e))
        transposed = (p.rng[:, 1] < p.rng[:, 0]).mean()
        assert 0.2 < transposed < 0.8                              # range blocks in both orientations
        lower = (p.tx_id[:, None] < p.recv_id[None, :]).mean()       # transmitter ids below AND above receiver ids
        assert 0.2 < lower < 0.8
        per_recv = np.bincount(p.rng[:, 0].astype(int), minlength=p.dim.size)[p.dim == 6]
        assert per_recv.min() >= 4 and per_recv.min() < nt          # a subset of the transmitters
        deg = np.bincount(np.concatenate([p.cv[:, :2].ravel(), p.rng[:, :2].ravel(), p.pri]).astype(int), minlength=p.dim.size)
        if name == "rocv_interleaved":    # both wave kernels: every transmitter and one receiver beyond 24 sources
            assert (deg[p.dim == 3] > 24).all() and (deg[p.dim == 6] > 24).sum() == 1
        # transmitters start off their true places, within a fraction of a range
        base = formats.slam2d_offsets(p.dim)
        off = np.linalg.norm(p.state[base[p.tx_id][:, None] + np.arange(3)] - p.truth["transmitters"], axis=1)
        assert np.allclose(off, 0.3) and p.rng[:, 2].min() > 10 * 0.3
        s = nonlinear.CRocv.from_problem(p)
        assert s.chi2() > 0
        # the prior: J = I, r = 0 whatever the state, chi2 0 -- it adds Omega to the diagonal block and nothing to eta
        g = s.linearize()[2]
        assert np.array_equal(g.J0, np.tile(np.eye(3).ravel(), (nt, 1))) and not g.r.any()


def test_gauss_newton_converges_on_the_fixtures():
    for name in ("rocv_small", "rocv_interleaved"):
        s = nonlinear.CRocv.from_problem(synth.make(name))
        n_it, norms, chi2 = rocv_ref.host_loop(s)
        print(name, n_it, norms, chi2)
        assert n_it <= 5 and norms[-1] <= 0.01, (name, norms)
        assert all(b <= a for a, b in zip(chi2, chi2[1:])) and chi2[-1] < 0.05 * chi2[0], (name, chi2)


def _golden_system(tmp_path):
    gold = np.load(GOLD)
    path = str(tmp_path / "g.txt")
    with open(path, "w") as f:
        f.write("\n".join(gold["lines"].tolist()) + "\n")
    return gold, formats.load_rocv_graph(path)


def test_loader_matches_the_reference_application(tmp_path):
    """the reference application on rocv_small (its own parser, CEdgeConstVelocity3D / CEdgePosVel_Landmark3D /
    CEdgeLandmark3DPrior): initial.txt, six decimals, pins load_rocv_graph -- the explicit vertices, the null vertex and
    CConstVelocity_Initializer --, and the initial chi2 it prints with two decimals pins the residuals of both groups, the
    information matrices as parsed and the prior's zero chi2."""
    gold, g = _golden_system(tmp_path)
    assert np.array_equal(g["dim"], gold["dim"]) and (~g["explicit"]).sum() == 5
    assert np.abs(g["state"] - gold["init"]).max() <= 5e-7 * max(1.0, np.abs(gold["init"]).max())
    assert abs(nonlinear.CRocv.from_problem(g).chi2() - float(gold["initial_chi2"])) <= 0.006


def test_loop_matches_the_reference_application(tmp_path):
    """CRocv with a dense float64 solve against the application's Gauss-Newton run (4 iterations, residual norms 3.9372
    0.1947 0.0216 0.0054, final chi2 73.33). Every Jacobian of this family is analytic in the reference too, and the
    priors take the gauge away, so -- unlike the 3D landmark golden -- the STATES are compared. Measured on the CPU, each
    bounded at 4 x the measured value, the factor tests/parity.py grants (a measured value below what the application's
    print-out resolves counts as that resolution: 5e-7 for solution.txt's six decimals, 5e-5 for the norms' four, 5e-3
    for chi2's two):
      measured                                      bound
      final states, max |difference|     5.0e-7     2e-6    (solution.txt's rounding)
      final chi2, |difference|           1.2e-3     2e-2    (73.3331 here, printed 73.33)
      residual norms, max |difference|   4.7e-5     2e-4    (printed with four decimals)"""
    gold, g = _golden_system(tmp_path)
    s = nonlinear.CRocv.from_problem(g)
    n_it, norms, chi2 = rocv_ref.host_loop(s, int(gold["max_iter"]), float(gold["threshold"]))
    d_state = np.abs(s.state - gold["final"]).max()
    d_chi2 = abs(s.chi2() - float(gold["final_chi2"]))
    d_norm = np.abs(np.array(norms) - gold["residual_norms"]).max() if n_it == gold["residual_norms"].size else np.inf
    print("iterations %d, states %.3e, chi2 %.6f vs %.2f (%.3e), norms %.3e" % (
        n_it, d_state, s.chi2(), float(gold["final_chi2"]), d_chi2, d_norm))
    assert n_it == gold["residual_norms"].size
    assert d_state <= 2e-6
    assert d_chi2 <= 2e-2
    assert d_norm <= 2e-4
