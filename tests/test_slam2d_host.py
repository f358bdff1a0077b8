"""Host side of 2D landmark SLAM: the text tokens (formats.load_slam2d_graph / save_slam2d_graph), the numpy
linearization of both edge groups and the synthetic fixtures. No GPU."""
import numpy as np

from slam_plus_plus_amd import formats, nonlinear, synth


def test_round_trip(tmp_path):
    p = synth.make("slam2d_interleaved")
    path = str(tmp_path / "g.txt")
    formats.save_slam2d_graph(path, p.dim, p.state, p.odo, p.odo_info, p.obs, p.obs_info, p.odo_seq, p.obs_seq)
    g = formats.load_slam2d_graph(path)
    assert np.array_equal(g["dim"], p.dim)
    # the file lists the edges in the global order; %.17g: every double comes back
    for grp in ("odo", "obs"):
        o = np.argsort(p[grp + "_seq"])
        for k in (grp, grp + "_info", grp + "_seq"):
            assert np.array_equal(g[k], p[k][o]), k
    base = formats.slam2d_offsets(p.dim)
    pose = np.flatnonzero(p.dim == 3)
    idx = base[pose][:, None] + np.arange(3)
    assert np.array_equal(g["state"][idx], p.state[idx])
    # landmarks have no vertex token: each comes back as the reference initialises it from its first observation
    first = {}
    for k in np.argsort(p.obs_seq):
        first.setdefault(int(p.obs[k, 1]), k)
    for l, k in first.items():
        ps = p.state[base[int(p.obs[k, 0])]:][:3]
        q = formats._se2_compose(ps, [p.obs[k, 2], 0.0, p.obs[k, 3]])
        assert np.array_equal(g["state"][base[l]:base[l] + 2], [np.hypot(q[0], q[1]), q[2]])


def test_token_handling(tmp_path):
    path = str(tmp_path / "t.txt")
    with open(path, "w") as f:
        f.write("VERTEX_SE2 0 1 2 0.5\n"
                "EDGE_SE2 0 1 1 0 0.25 10 0 0 20 0 30\n"           # pose 1 initialised by composing the odometry
                "EDGE_SE2_XY 0 2 3 4 7 1 9\n"                       # XY: polar measurement, information -> identity
                "LANDMARK2:RB 1 3 2 0.1 5 0.5 6\n"                  # RB: measurement and information kept
                "LANDMARK 2 1 0.5 0.5 1 0 1\n"                      # the landmark named first: swapped
                "EDGE_BEARING_SE2_XY 4 2 1 1 1 0 1\n"               # unknown first vertex, known landmark second: a new pose
                "# comment\n")
    g = formats.load_slam2d_graph(path)
    assert g["dim"].tolist() == [3, 3, 2, 2, 3]
    assert np.array_equal(g["odo"], [[0, 1, 1, 0, 0.25]]) and np.array_equal(g["odo_info"][0], [[10, 0, 0], [0, 20, 0], [0, 0, 30]])
    assert np.array_equal(g["odo_seq"], [0]) and np.array_equal(g["obs_seq"], [1, 2, 3, 4])
    assert np.array_equal(g["obs"][:, :2], [[0, 2], [1, 3], [1, 2], [4, 2]])
    assert np.allclose(g["obs"][0, 2:], [5.0, np.arctan2(4, 3)], rtol=0, atol=1e-15)
    assert np.array_equal(g["obs_info"][0], np.eye(2)) and np.array_equal(g["obs_info"][2], np.eye(2))
    assert np.array_equal(g["obs"][1, 2:], [2, 0.1]) and np.array_equal(g["obs_info"][1], [[5, 0.5], [0.5, 6]])
    base = formats.slam2d_offsets(g["dim"])
    x = g["state"]
    c, s = np.cos(0.5), np.sin(0.5)
    p1 = np.array([1 + c, 2 + s, 0.75])
    assert np.allclose(x[base[1]:base[1] + 3], p1, rtol=0, atol=1e-15)
    assert np.allclose(x[base[2]:base[2] + 2], [1 + c * 3 - s * 4, 2 + s * 3 + c * 4], rtol=0, atol=1e-15)    # XY initialiser
    q = p1[:2] + 2 * np.array([np.cos(0.75), np.sin(0.75)])                                                   # RB initialiser, as written
    assert np.allclose(x[base[3]:base[3] + 2], [np.hypot(*q), 0.85], rtol=0, atol=1e-15)
    assert np.array_equal(x[base[4]:base[4] + 3], [0, 0, 0])                                                  # the null vertex
    assert np.array_equal(formats.load_graph(path)["se2_edges"], [[0, 1, 1, 0, 0.25]])                        # load_graph: as before


def test_jacobians_against_central_differences():
    p = synth.make("slam2d_small")
    args = (p.odo, p.odo_info, p.obs, p.obs_info)
    groups = formats.slam2d_linearize(p.dim, p.state, *args)
    base = formats.slam2d_offsets(p.dim)
    h = 1e-6
    for gi, g in enumerate(groups):
        for side, (v, d, J) in enumerate(((g.v0, g.d0, g.J0), (g.v1, g.d1, g.J1))):
            J = J.reshape(-1, d, g.rd).transpose(0, 2, 1)                      # (edge, rd, d)
            num = np.empty_like(J)
            for c in range(d):                                                 # edge by edge: neighbours share vertices
                r = []
                for sgn in (1, -1):
                    res = np.empty((g.v0.size, g.rd))
                    for e in range(g.v0.size):
                        x = p.state.copy()
                        x[base[v[e]] + c] += sgn * h
                        res[e] = formats.slam2d_linearize(p.dim, x, *_only(args, gi, e))[gi].r[0]
                    r.append(res)
                num[:, :, c] = -(r[0] - r[1]) / (2 * h)                        # r = z - h(x)
            assert np.abs(num - J).max() <= 1e-6 * np.abs(J).max(), (gi, side)


def _only(args, gi, e):
    odo, odo_info, obs, obs_info = args
    if gi == 0:
        return odo[e:e + 1], odo_info[e:e + 1], obs[:0], obs_info[:0]
    return odo[:0], odo_info[:0], obs[e:e + 1], obs_info[e:e + 1]


def test_fixtures_are_what_the_issue_describes():
    for name, (n_poses, n_lm) in (("slam2d_small", (60, 90)), ("slam2d_interleaved", (150, 300))):
        p = synth.make(name)
        assert (p.dim == 3).sum() == n_poses and (p.dim == 2).sum() == n_lm and p.dim[0] == 3 and p.unary_vertex == 0
        assert p.odo.shape[0] == n_poses - 1 + n_poses // 5
        per_lm = np.bincount(p.obs[:, 1].astype(int), minlength=p.dim.size)[p.dim == 2]
        assert per_lm.min() >= 2 and per_lm.max() <= 5
        assert np.array_equal(np.sort(np.concatenate([p.odo_seq, p.obs_seq])), np.arange(p.odo.shape[0] + p.obs.shape[0]))
        interleaved = (p.obs[:, 1] < p.obs[:, 0]).any()
        assert interleaved == (name == "slam2d_interleaved")
        s = nonlinear.CSlam2D.from_problem(p)
        x0 = s.state.copy()
        s.plus(np.zeros(x0.size))
        assert np.array_equal(s.state, x0) and s.chi2() > 0
    # the existing names keep their output
    assert synth.make("lm2d_small").v0.size == synth.landmark2d_problem(80, 200, 32).v0.size


def _dense_solve(groups, first):
    """Lambda and eta of all groups in dense float64 + the unit unary factor, numpy solve"""
    dim = groups[0].dim
    base = formats.slam2d_offsets(dim)
    n = int(base[-1])
    L, eta = np.zeros((n, n)), np.zeros(n)
    for g in groups:
        J0 = g.J0.reshape(-1, g.d0, g.rd).transpose(0, 2, 1)
        J1 = g.J1.reshape(-1, g.d1, g.rd).transpose(0, 2, 1)
        Om = g.Om.reshape(-1, g.rd, g.rd)
        for e in range(g.v0.size):
            sa, sb = slice(base[g.v0[e]], base[g.v0[e]] + g.d0), slice(base[g.v1[e]], base[g.v1[e]] + g.d1)
            A, B = J0[e].T @ Om[e], J1[e].T @ Om[e]
            L[sa, sa] += A @ J0[e]
            L[sb, sb] += B @ J1[e]
            L[sa, sb] += A @ J1[e]
            L[sb, sa] += B @ J0[e]
            eta[sa] += A @ g.r[e]
            eta[sb] += B @ g.r[e]
    u = groups[0].unary_vertex
    L[base[u]:base[u + 1], base[u]:base[u + 1]] += np.eye(dim[u])
    return True, np.linalg.solve(L, eta)


def test_loader_and_loop_match_the_reference_application(tmp_path):
    """tests/golden/slam2d_gn.npz (tools/make_golden_slam2d.py): the reference application on an EDGE_SE2 / EDGE_SE2_RB
    file. Its initial states -- poses composed from the odometry, landmarks as its range-bearing initializer leaves
    them -- and initial chi2 pin load_slam2d_graph; its five Gauss-Newton iterations (which do not converge from that
    start) pin CSlam2D + the loop: residual norms to the 4 decimals it prints, states within the bound of the se2 loop
    golden (tests/test_nonlinear_gn.py:57-58) + the 5e-7 of the 6 decimals it writes."""
    import os
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "slam2d_gn.npz"))
    path = str(tmp_path / "g.txt")
    with open(path, "w") as f:
        f.write("\n".join(gold["lines"].tolist()) + "\n")
    s = nonlinear.CSlam2D.from_problem(formats.load_slam2d_graph(path))
    assert np.abs(s.state - gold["init"]).max() <= 5e-7 * max(1.0, np.abs(gold["init"]).max())
    assert abs(s.chi2() - float(gold["initial_chi2"])) <= 0.006            # printed with two decimals
    norms = []
    for _ in range(int(gold["max_iter"])):
        class _Path:
            solve = staticmethod(_dense_solve)
        solver = nonlinear.CNonlinearSolver_Lambda(s, path=_Path())
        solver.Optimize(1, float(gold["threshold"]))
        norms.append(solver.last_dx_norm)
    assert np.abs(np.array(norms) - gold["residual_norms"]).max() <= 6e-5 * max(1.0, gold["residual_norms"].max())
    d = np.abs(s.state - gold["final"]).max()
    assert d <= 1e-6 * max(1.0, np.abs(gold["final"]).max()) + 5e-7, d
