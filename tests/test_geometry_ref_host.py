"""The geometry fixture (tests/golden/geometry_edges.npz) and what stands behind its tolerances, host only (DESIGN.md
section 18): the committed file is what tools/make_golden_geom_edges.py generates; every branch cell of spp_geometry.hip is
hit, asserted from the branch table the 50-digit reference recorded; every threshold sits where the choice of arm is below
the tolerance (or, where the arms differ by design, far above it); the float64 mirrors of formats.py agree with the
reference within the quotients that set the constants c of tests/geometry_cases.py."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import geometry_cases as gc
import geometry_mirrors as gm
import geometry_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _gold():
    return gm.load()


@functools.lru_cache(maxsize=None)
def _tool():
    spec = importlib.util.spec_from_file_location("make_golden_geom_edges", os.path.join(ROOT, "tools", "make_golden_geom_edges.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _tol(g, fam):
    """{output: (n, width) c eps scale}"""
    return {k: gc.C[fam][k] * gc.EPS * v for k, v in gc.SCALES[fam](g).items()}


def test_fixture_is_what_the_tool_generates():
    g, new = _gold(), _tool().generate()
    assert sorted(g) == sorted(new)
    for k in g:
        assert g[k].dtype == new[k].dtype and g[k].shape == new[k].shape, k
        assert np.array_equal(g[k], new[k]), k
    assert os.path.getsize(gm.GOLD) < 128 << 10      # well below the larger goldens


def test_case_builder_is_numpy_only_and_deterministic():
    a, b = gc.inputs(), gc.inputs()
    assert all(np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in a)
    assert all(np.array_equal(a[k], _gold()[k]) for k in a)


def test_every_rotation_that_passes_through_log_stays_1e_3_from_pi():
    g = _gold()
    for name, th in (("se3 expectation", g["se3_aux"][:, 0]), ("se3 residual", g["se3_aux"][:, 1]), ("composition", g["plus_aux"][:, 0])):
        assert (np.pi - th >= 1e-3).all(), (name, th.max())
    assert np.pi - g["se3_aux"][:, 0].max() < 1.01e-3          # ... and one case goes that far


def test_every_coverage_cell_is_hit():
    g = _gold()
    br = lambda fam, col: gm.br(g, fam, col)
    # axis_angle_to_rot / aa_to_quat: all eight cells of the angle through every kernel that calls them
    for fam, cols in (("se3", ("cell1", "cell2", "cellz")), ("xyz", ("cell",)), ("ba", ("cell",)), ("stereo", ("cell",)),
                      ("plus", ("cell_p", "cell_d"))):
        for col in cols:
            assert set(range(8)) <= set(br(fam, col)), (fam, col, sorted(set(br(fam, col))))
    # SE(3) edge: relative rotation
    the, thr, we, wr, vne, vnr = g["se3_aux"].T
    assert (br("se3", "vn_e_tiny") & (vne == 0)).any() and (br("se3", "vn_e_tiny") & (vne > 0)).any()    # th_e = 0; 0 < vn < 1e-12
    js = br("se3", "jr_series")
    assert ((the > 0) & (the < 0.98e-4) & (js == 1)).any()
    assert ((the > 0.98e-4) & (the < 1e-4) & (js == 1)).any() and ((the > 1e-4) & (the < 1.02e-4) & (js == 0)).any()
    assert ((the > 0.1) & (the < 3.0)).any() and ((np.pi - the > 1e-3) & (np.pi - the < 1.01e-3)).any()
    assert (br("se3", "w_e_neg") == 1).any() and ((br("se3", "w_e_neg") == 0) & (the > 0.1)).any()
    # ... residual rotation: 0, about 1, 3.0, both signs of w at a large angle
    assert (br("se3", "vn_r_tiny") & (vnr == 0)).any() and (br("se3", "vn_r_tiny") & (vnr > 0)).any()
    assert (np.abs(thr - 1.0) < 0.05).any()
    for neg in (0, 1):
        assert ((br("se3", "w_r_neg") == neg) & (np.abs(thr - 3.0) < 1e-9)).any(), neg
    # ... translations of magnitude 1e-3, 1, 1e3
    P, E = g["se3_poses"], g["se3_edges"]
    dt = np.linalg.norm(P[E[:, 1].astype(int), :3] - P[E[:, 0].astype(int), :3], axis=1)
    assert ((dt > 1e-4) & (dt < 1e-2)).any() and ((dt > 0.1) & (dt < 10)).any() and (dt > 300).any()
    # ... gathers: a repeated id, an edge to itself, ids in both orders
    assert (E[:, 0] == E[:, 1]).any() and (E[:, 0] > E[:, 1]).any() and (E[:, 0] < E[:, 1]).any()
    assert np.bincount(E[:, :2].astype(int).ravel()).max() >= 3
    # composition
    assert (br("plus", "d_zero") == 1).sum() >= 2 and ((br("plus", "d_zero") == 1) & (br("plus", "cell_p") == 6)).any()
    assert (br("plus", "cell_d") == 1).any()                                                   # |dr| < 1e-12
    vn = g["plus_aux"][:, 2]
    assert (br("plus", "vn_tiny") & (vn == 0)).any() and (br("plus", "vn_tiny") & (vn > 0)).any()
    assert ((vn > 1e-12) & (vn < 1e-8)).any()
    assert (br("plus", "w_neg") == 1).sum() >= 2 and (br("plus", "cell_p") >= 6).any()
    # 2D pose-pose edge
    for col in ("a1_outside", "a2_outside", "a1_neg", "a2_neg", "near_plus_pi", "near_minus_pi"):
        assert (br("se2", col) == 1).any() and (br("se2", col) == 0).any(), col
    assert set(br("se2", "err_arm")) == {0, 1, 2}
    assert np.abs(np.abs(g["se2_r"][:, 2]) - np.pi).min() > 1e-7                               # near pi, not on it
    # range-bearing edge
    d = g["rb_aux"][:, 0]
    assert (br("rb", "d_zero") == 1).any() and ((d > 0) & (d < 1e-5) & (br("rb", "floored") == 1)).any()
    assert ((d > 1e-5) & (d < 3e-5) & (br("rb", "floored") == 0)).any() and (d > 1).any()
    assert (br("rb", "atan_near_cut_pos") == 1).any() and (br("rb", "atan_near_cut_neg") == 1).any()
    assert set(br("rb", "err_arm")) == {0, 1, 2} and (br("rb", "a_outside") == 1).any()
    # mono BA
    intr, obs = g["ba_intr"], g["ba_obs"]
    assert (br("ba", "k_zero") == 1).any() and (np.abs(g["ba_aux"][:, 3] - 0.3) < 0.03).any()
    assert (intr[:, 0] != intr[:, 1]).all() and (br("ba", "on_axis") == 1).any() and (br("ba", "behind") == 1).any()
    Xn = np.linalg.norm(g["ba_pts"][obs[:, 1].astype(int)], axis=1)
    assert ((Xn > 500) & (br("ba", "cell") <= 4) & (br("ba", "cell") >= 1)).any()
    # stereo
    for col in ("k_zero", "b_zero", "rho_l_zero", "rho_r_zero", "rho_l_tiny"):
        assert (br("stereo", col) == 1).any(), col
    # gathers of the offset kernels: offsets that are no multiple of the vertex width
    for fam, w in (("xyz", 6), ("rb", 3)):
        base = gc.offsets(g[fam + "_dim"])
        po = base[g[fam + "_obs"][:, 0].astype(int)]
        assert (po % w != 0).any()
        assert np.bincount(g[fam + "_obs"][:, 0].astype(int)).max() >= 2 and np.bincount(g[fam + "_obs"][:, 1].astype(int)).max() >= 2
    for fam in ("ba", "stereo"):
        o = g[fam + "_obs"]
        assert np.bincount(o[:, 0].astype(int)).max() >= 3 and np.bincount(o[:, 1].astype(int)).max() >= 3
        assert (np.diff(o[:, 0]) < 0).any() and (np.diff(o[:, 0]) > 0).any()


def test_mirrors_agree_with_the_reference_and_set_c():
    """The largest |mirror - reference| / (eps scale) per family and output; c is 8 x that (a quotient below 1 counts as 1),
    rounded up to a power of two, at most 4096; a case whose mirror quotient alone exceeds 512 would be ill-conditioned.
    Measured: se3 1.12 / 0.59 / 0.63 (J0 / J1 / r), xyz 0.56 / 0.50 / 0.46, ba 0.17 / 0.17 / 0.03, stereo 0.68 / 0.68 /
    0.15, se2 0.77 / 0 / 0.82, rb 0.65 / 0.65 / 0.29, composition 0.75 (vector) / 0.46 (matrix), 2D update 0.25; slam2d_linearize and
    slam3d_plus give the quotients of se2_linearize and se3_plus."""
    g = _gold()
    m = gm.mirrors(g)
    m["upd2"] = {"out": np.concatenate([(g["upd2_p"] + g["upd2_d"])[:, :2], np.fmod(g["upd2_p"][:, 2:] + g["upd2_d"][:, 2:], gc.TWO_PI)], axis=1)}
    for key, got in m.items():
        fam = key.split("_")[0]
        q = {k: v.max() for k, v in gm.quotients(g, fam, got).items()}
        print(key, " ".join("%s %.3g" % kv for kv in q.items()))
        for name, v in q.items():
            c = gc.C[fam][name]
            assert v <= 512, (key, name, v)
            assert c <= 4096 and c & (c - 1) == 0
            assert gc.c_rule(v) <= c <= 2 * gc.c_rule(v), (key, name, v, c)
    # the landmarks of slam3d_plus: the plain sum
    st, dx, _ = gm.interleave(g["plus_p"], g["plus_d"], 3)
    assert np.array_equal(m["plus_slam3d"]["lm"], (st + dx).reshape(-1, 9)[:, 6:])


# ---- threshold placement: both arms of every choice, evaluated at 50 digits on the cases next to the threshold
def _kernel_forms(g, arms, guard=True):
    """{family: [per case {output: array}]} of the kernel forms under `arms`"""
    out = {}
    P, E = g["se3_poses"], g["se3_edges"]
    out["se3"] = [gr.k_se3_edge(P[int(e[0])], P[int(e[1])], e[2:8], arms) for e in E]
    x, base = g["xyz_state"], gc.offsets(g["xyz_dim"])
    out["xyz"] = [gr.k_xyz_edge(x[base[int(o[0])]:base[int(o[0])] + 6], x[base[int(o[1])]:base[int(o[1])] + 3], o[2:5], arms)
                  for o in g["xyz_obs"]]
    for fam in ("ba", "stereo"):
        out[fam] = [gr.k_proj_edge(g[fam + "_cams"][int(o[0])], g[fam + "_intr"][int(o[0])], g[fam + "_pts"][int(o[1])], o[2:],
                                   fam == "stereo", arms, guard) for o in g[fam + "_obs"]]
    out["plus"] = [gr.k_plus(p, d, arms) for p, d in zip(g["plus_p"], g["plus_d"])]
    return out


@functools.lru_cache(maxsize=None)
def _own():
    return _kernel_forms(_gold(), None)


def _moved(g, a, b, fam):
    """per case: the largest |a - b| / tolerance over the family's outputs"""
    tol = _tol(g, fam)
    return np.array([max((gr.absdiff(x[k], y[k]) / tol[k][i]).max() for k in tol) for i, (x, y) in enumerate(zip(a[fam], b[fam]))])


def test_kernel_forms_are_the_reference():
    """the kernel's algorithm (analytic Jacobians, quaternion logarithm, x - b e0), evaluated at 50 digits, IS the model's
    central difference: to the single rounding of the fixture (and 1e-9 of the tolerance, where the 50th digit divided by
    h = 1e-20 shows in an entry that is exactly zero). What remains for the GPU test is float64 arithmetic."""
    g = _gold()
    for fam, cases in _own().items():
        tol = _tol(g, fam)
        for i, c in enumerate(cases):
            for k in tol:
                if fam == "plus" and k == "out" and gm.pi_crossing(g)[i]:
                    assert gr.absdiff(c[k][:3], g["plus_out"][i, :3]).max() <= 0.51 * gc.EPS * np.abs(g["plus_out"][i, :3]).max()
                    continue
                ref = g[fam + "_" + k][i]              # rounded once: half an ulp of itself is all that may separate them
                assert (gr.absdiff(c[k], ref) <= 0.51 * gc.EPS * np.abs(ref) + 1e-9 * tol[k][i]).all(), (fam, i, k)


@pytest.mark.parametrize("name, lo, hi", [("TH_ROT", 0.98e-6, 1.02e-6), ("TH_QUAT", 1e-13, 1e-8), ("TH_VN", 1e-14, 1e-8),
                                          ("TH_JR", 0.98e-4, 1.02e-4)])
def test_small_argument_thresholds_sit_below_the_tolerance(name, lo, hi):
    """Moving the threshold to either side of the cases next to it -- so that each of them is evaluated by the series AND by
    the closed form -- moves no output by 1/8 of its tolerance (measured: at most 5.5e-12 of it, TH_QUAT)."""
    g = _gold()
    a, b = _kernel_forms(g, {name: lo}), _kernel_forms(g, {name: hi})
    worst, switched = 0.0, 0
    for fam in a:
        m = _moved(g, a, b, fam)
        worst, switched = max(worst, m.max()), switched + int((m > 0).sum())
        assert (m < 0.125).all(), (fam, m)
    print(name, "cases that changed arm: %d, largest move / tolerance: %.3g" % (switched, worst))
    assert switched >= 2 and worst > 0   # cases on both sides took the other arm (at 50 digits the move is never exactly 0)


def test_sign_flips_that_matter_and_those_that_do_not():
    """quat_to_aa's w < 0 flip decides the representative: without it every case with a negative w moves by far more than 10
    tolerances. The c < 0 flip of aa_to_quat and the flip of the conjugate in the SE(3) error only hand quat_to_aa the other
    sign of the same rotation: switching them off changes nothing (below 1/8 tolerance)."""
    g = _gold()
    own = _own()
    off = _kernel_forms(g, {"no_w_flip": True})
    neg = {"se3": (gm.br(g, "se3", "w_e_neg") | gm.br(g, "se3", "w_r_neg")) == 1, "plus": gm.br(g, "plus", "w_neg") == 1}
    for fam, sel in neg.items():
        tol = _tol(g, fam)
        outs = [k for k in tol if k != "R"]                    # the rotation MATRIX is the same for both representatives
        m = np.array([max((gr.absdiff(x[k], y[k]) / tol[k][i]).max() for k in outs) for i, (x, y) in enumerate(zip(own[fam], off[fam]))])
        assert sel.sum() >= 2 and (m[sel] > 10).all() and (m[~sel] == 0).all(), (fam, m)
    for name in ("no_quat_flip", "no_qec_flip"):
        other = _kernel_forms(g, {name: True})
        for fam in ("se3", "plus"):
            assert (_moved(g, own, other, fam) < 0.125).all(), (name, fam)


def test_range_floor_and_rho_guard_are_arms_by_design():
    g = _gold()
    x, base, obs = g["rb_state"], gc.offsets(g["rb_dim"]), g["rb_obs"]
    tol = _tol(g, "rb")
    floored = gm.br(g, "rb", "floored") == 1
    for i, o in enumerate(obs):
        p, l = x[base[int(o[0])]:base[int(o[0])] + 3], x[base[int(o[1])]:base[int(o[1])] + 2]
        J0, J1, r, _, _ = gr.rb_edge(p, l, o[2:4], floor=False)
        if J0 is None:                                         # d = 0 without the floor: no finite Jacobian at all
            assert floored[i] and gm.br(g, "rb", "d_zero")[i]
            assert np.abs(r - g["rb_r"][i]).max() > 10 * tol["r"][i].max()
            continue
        m = max((np.abs(J0 - g["rb_J0"][i]) / tol["J0"][i]).max(), (np.abs(r - g["rb_r"][i]) / tol["r"][i]).max())
        assert (m > 10) if floored[i] else (m < 0.125), (i, m)
    assert floored.sum() >= 2
    # the rho > 0 tests of the stereo kernel: without them rho = 0 divides zero by zero
    zero = (gm.br(g, "stereo", "rho_l_zero") | gm.br(g, "stereo", "rho_r_zero")) == 1
    bare = _kernel_forms({k: v for k, v in g.items()}, None, guard=False)["stereo"]
    assert zero.sum() >= 2 and all((b is None) == bool(z) for b, z in zip(bare, zero))
    own = _own()["stereo"]
    assert all(a[k] == b[k] for a, b, z in zip(own, bare, zero) if not z for k in a)
