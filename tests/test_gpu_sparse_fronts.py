"""The supernodal multifrontal Cholesky of csrc/spp_sparse.hip, front class by front class, against a float64 reference
refined in longdouble, on the designed systems of tests/sparse_fixtures.py (clique forests and clique trees whose fronts
are chosen, not left to the ordering of a pose graph).

One child process per variant of the run-time switches (read once per process), one after the other; a child
(tests/sparse_fronts_child.py) solves every designed system and writes x and the front table
(Context.sparse_fronts()). This process asserts
  coverage   from the front tables of all children together: every size class as childless root, parent and child, both
             sides of every class boundary, the pivot paddings, child layout x parent kind, the thresholds of the backward
             kernels, the tree shapes, the team sizes. A missing cell fails with its name: change the fixture, not the list.
  accuracy   |x - x_ref| <= 1e-12 |x_ref| per connected component (the bound of test_tiny_ragged_and_disconnected_systems;
             cond_2 <= 100 by design, tests/test_sparse_fixtures_host.py) and a relative residual <= 1e-11, printed beside
             LAPACK's own error on the same systems
  bits       a repeated solve, a solve after another right-hand side, SPP_DAG_SPLIT=2 against the default, SPP_SPARSE_DAG=0
             against the default where no front is of class 4 or higher than 192 rows, SPP_DAG_TIMEOUT_TICKS=1 against
             SPP_SPARSE_DAG=0
  failures   a negative pivot inside a class-2, class-3 and class-4 clique and a NaN inside the class-4 one: reported, the
             right-hand side untouched, the same solver object then solves the healthy system within the bound."""
import os
import subprocess
import sys

import numpy as np
import pytest

import sparse_fixtures as sf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "sparse_fronts_child.py")

NO_AMALG = {"SPP_AMALG_SMALL": "0", "SPP_AMALG_ZEROS": "0", "SPP_AMALG_ZEROS_SMALL": "0"}
# variant -> (switches, fixtures, failure paths too)
VARIANTS = {
    "default": ({}, sf.NAMES, True),
    "levels": ({"SPP_SPARSE_DAG": "0"}, sf.NAMES, False),
    "noteams": ({"SPP_SPARSE_TEAMS": "0"}, sf.NAMES, True),
    "split": ({"SPP_DAG_SPLIT": "2"}, sf.NAMES, False),
    "mid128": ({"SPP_MID_FRONT_MAX": "128"}, sf.NAMES, False),
    "mid640": ({"SPP_MID_FRONT_MAX": "640"}, sf.NAMES, False),
    "team2": ({"SPP_SPARSE_TEAM_MAX": "2", "SPP_SPARSE_TEAM_COLS": "256"}, sf.NAMES, False),
    "teamcols8": ({"SPP_SPARSE_TEAM_COLS": "8"}, sf.NAMES, False),
    "timeout": ({"SPP_DAG_TIMEOUT_TICKS": "1"}, sf.NAMES, False),
}
MID = {"mid128": 128, "mid640": 640}                 # SPP_MID_FRONT_MAX of a variant (default 320)
HOST_DRIVEN = ("levels", "noteams", "timeout")       # variants whose class-4 fronts go through the host-driven dense factor
TEAM_MAX_DEFAULT = 40                                # SPP_SPARSE_TEAM_MAX; half the device's CU count bounds it further
# (fixture, clique width, value): one diagonal scalar of a pivot inside a clique of class 2, 3 and 4
FAILURES = [("forest_a", 112, "negative"), ("forest_a", 192, "negative"), ("forest_b", 384, "negative"), ("forest_b", 384, "nan")]


def _child(tmp, tag, env_extra, args):
    out = tmp / (tag + ".npz")
    env = dict(os.environ)
    for k in list(env):
        if k.startswith("SPP_") and k != "SPP_LIB":
            del env[k]
    env.update(env_extra)
    r = subprocess.run([sys.executable, CHILD, str(tmp / "inputs.npz"), str(out)] + args, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, "%s: exit %d\n%s%s" % (tag, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return dict(np.load(out))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sparse_fronts")
    fixtures = {name: sf.build(name) for name in sf.NAMES}
    inputs, ref = {}, {}
    fail_tags = []
    for name, fx in fixtures.items():
        lam = fx.lam
        for k in ("dim", "col_ptr", "row_idx", "blk_off", "vals"):
            inputs["%s/%s" % (name, k)] = getattr(lam, k)
        inputs[name + "/eta"] = fx.eta
        inputs[name + "/eta2"] = np.random.default_rng(11).normal(size=lam.n)
        ref[name] = (sf.reference(fx)[0], sf.lapack_solution(fx))
    for (name, width, what) in FAILURES:
        fx = fixtures[name]
        blocks = sf.clique_of_width(fx, width)["blocks"]
        v = int(blocks[blocks.size // 2])
        d = int(fx.lam.dim[v])
        off = int(fx.lam.blk_off[sf.diagonal_block(fx, v)]) + d * d - 1          # the block's last diagonal scalar
        tag = "%s:%d:%s" % (name, width, what)
        fail_tags.append(tag)
        inputs["fail_offset/" + tag] = np.int64(off)
        inputs["fail_value/" + tag] = np.float64(np.nan if what == "nan" else -abs(fx.lam.vals[off]))
    inputs["fail_tags"] = np.array(fail_tags)
    np.savez(tmp / "inputs.npz", **inputs)
    out = {}
    for tag, (switches, names, fail) in VARIANTS.items():          # one after the other, never side by side
        out[tag] = _child(tmp, tag, dict(NO_AMALG, **switches), ["designed", ",".join(names)] + (["fail"] if fail else []))
    out["amalg"] = _child(tmp, "amalg", {}, ["designed", ",".join(sf.TREE_NAMES)])
    for o in ("nd", "amd"):
        out[o] = _child(tmp, o, {"SPP_ORDERING": o}, ["pose"])
    return dict(fixtures=fixtures, ref=ref, out=out)


def _tables(runs):
    """(variant, system, dict of front arrays) of every front table of every child"""
    for tag, res in runs["out"].items():
        for name in sorted(set(k.split("/")[0] for k in res if "/front_h" in k)):
            yield tag, name, {k: res["%s/front_%s" % (name, k)].astype(np.int64) for k in ("h", "w", "pad", "cls", "level", "parent", "team")}


def _hp16(t):
    w16 = (t["w"] + 15) & ~15
    return (w16 + (t["h"] - t["w"]) + 15) & ~15


def test_front_tables_are_consistent(runs):
    """the table against the rules of sparse_analyze, and the forest against its design: one front per clique"""
    for tag, name, t in _tables(runs):
        mid = MID.get(tag, 320)
        hp16 = _hp16(t)
        cls = np.where(hp16 <= 32, 0, np.where(hp16 <= 64, 1, np.where(hp16 <= 128, 2, np.where(hp16 <= mid, 3, 4))))
        assert np.array_equal(t["cls"], cls), (tag, name)
        w16 = (t["w"] + 15) & ~15
        w128 = (t["w"] + 127) & ~127
        assert np.array_equal(t["pad"], np.where(cls == 4, w128 - t["w"], np.where(cls == 3, w16 - t["w"], 0))), (tag, name)
        has_parent = t["parent"] >= 0
        assert np.all(t["parent"][has_parent] > np.flatnonzero(has_parent)), "children come first"
        assert np.all(t["level"][t["parent"][has_parent]] > t["level"][has_parent])
        assert np.all((t["h"] - t["w"] == 1) == ~has_parent), "a root holds its pivots and the right-hand-side slot alone"
        assert np.all((t["team"] > 1) <= (cls == 4))
        assert int(runs["out"][tag][name + "/levels"]) == t["level"].max() + 1
        if name in sf.NAMES:
            assert t["w"].sum() == runs["fixtures"][name].lam.n
        if name in sf.FOREST_WIDTHS:      # one childless root per clique, and the root of the forest's small tree
            n_children = np.bincount(t["parent"][has_parent], minlength=t["h"].size)
            assert sorted(t["w"][~has_parent & (n_children == 0)]) == sorted(sf.FOREST_WIDTHS[name]), (tag, name)
            assert np.sum(~has_parent) == len(sf.FOREST_WIDTHS[name]) + 1


def test_designed_leaves_stay_fronts_without_amalgamation(runs):
    """with the amalgamation switches at zero only zero-fill merges happen: every designed leaf is a front of its own"""
    for name in sf.TREE_NAMES:
        fx = runs["fixtures"][name]
        res = runs["out"]["default"]
        w = sorted(int(v) for v in res[name + "/front_w"])
        for g in fx.cliques:
            if g["role"] == "separator":      # and a separator is one front: every leaf went before any of its blocks
                assert g["width"] in w, (name, g["width"], w)
            if g["role"] == "leaf":
                assert g["width"] in w, (name, g["width"], w)
                w.remove(g["width"])


def test_both_block_orientations_occur(runs):
    """a stored block (i < j) is transposed on its way into the front iff the permutation puts i behind j"""
    for name in sf.NAMES:
        lam = runs["fixtures"][name].lam
        order = runs["out"]["default"][name + "/order"]
        inv = np.empty(lam.nb, dtype=np.int64)
        inv[order] = np.arange(lam.nb)
        off = lam.row_idx != lam.col_idx
        flipped = inv[lam.row_idx[off]] > inv[lam.col_idx[off]]
        assert flipped.any() and (~flipped).any(), name


def _coverage(runs, cu_count):
    cells = {}

    def cell(key, hit=False):
        cells[key] = cells.get(key, False) or bool(hit)

    team_cap = min(TEAM_MAX_DEFAULT, cu_count // 2)
    layouts = ("classes 0-2", "class 3", "class 4")
    for tag, name, t in _tables(runs):
        h, w, cls, parent, team, level = t["h"], t["w"], t["cls"], t["parent"], t["team"], t["level"]
        hp16 = _hp16(t)
        n_children = np.bincount(parent[parent >= 0], minlength=h.size)
        kid = parent >= 0
        for c in range(5):
            cell("class %d as a childless root" % c, np.any((cls == c) & ~kid & (n_children == 0)))
            cell("class %d as a parent" % c, np.any((cls == c) & (n_children > 0)))
            cell("class %d as a child" % c, np.any((cls == c) & kid))
            cell("class %d with w %% 16 == 0" % c, np.any((cls == c) & (w % 16 == 0)))
            cell("class %d with w %% 16 == 1" % c, np.any((cls == c) & (w % 16 == 1)))
        for v in (32, 48, 64, 80, 128, 144):
            cell("hp16 == %d" % v, np.any(hp16 == v))
        for mid, where in ((128, "mid128"), (320, "default"), (640, "mid640")):      # each in the child that sets it
            cell("SPP_MID_FRONT_MAX=%d: hp16 == %d, the last below class 4" % (mid, mid), tag == where and np.any((hp16 == mid) & (cls < 4)))
            cell("SPP_MID_FRONT_MAX=%d: hp16 == %d, the first of class 4" % (mid, mid + 16), tag == where and np.any((hp16 == mid + 16) & (cls == 4)))
        cell("class 4 with w % 128 == 0", np.any((cls == 4) & (w % 128 == 0)))
        cell("class 4 with w % 128 == 1", np.any((cls == 4) & (w % 128 == 1)))
        cell("class 3 with pad 15", np.any((cls == 3) & (t["pad"] == 15)))
        cell("a front with w == 1", np.any(w == 1))
        # child layout x parent kind
        lay = np.minimum(np.maximum(cls, 2), 4) - 2
        for c in np.flatnonzero(kid):
            p = parent[c]
            if cls[p] < 4:
                kind = layouts[lay[p]]
            else:
                kind = "class-4 host-driven" if tag in HOST_DRIVEN else "class-4 team"
                assert (team[p] >= 2) == (tag != "noteams")
            cells["child layout %s under parent %s" % (layouts[lay[c]], kind)] = True
        for lc in layouts:
            for kind in layouts[:2] + ("class-4 team", "class-4 host-driven"):
                cell("child layout %s under parent %s" % (lc, kind))
        cell("border h - w == 1", np.any(h - w == 1))
        cell("border h - w > w", np.any(h - w > w))
        for r in (0, 1, 63):
            cell("backward: w %% 64 == %d" % r, np.any(w % 64 == r))
        for v in (192, 193, 1024, 1025):
            cell("backward: h == %d" % v, np.any(h == v))
        cell("backward: (h - w) % 8 != 0", np.any((h - w) % 8 != 0))
        cell("a tree of at least 3 levels", level.max() >= 2)
        cell("a parent with at least 64 children", n_children.max() >= 64)
        cell("at least 2 roots in one system", np.sum(~kid) >= 2)
        cell("the split launch has both parts (SPP_DAG_SPLIT=2: a class >= 2 front above a level of fronts of at most 64 rows)",
             tag == "split" and np.any(cls >= 2) and level[cls >= 2].min() >= 1)
        cell("team size 2", np.any(team == 2))
        cell("team size %d, the largest the device allows" % team_cap, np.any(team == team_cap))
        cell("a team size between 2 and %d" % team_cap, np.any((team > 2) & (team < team_cap)))
        assert team.max() <= team_cap
    return cells


def test_every_coverage_cell_is_filled(runs):
    import torch
    cells = _coverage(runs, torch.cuda.get_device_properties(0).multi_processor_count)
    missing = sorted(k for k, hit in cells.items() if not hit)
    print("%d coverage cells" % len(cells))
    assert not missing, "coverage cells without a front: " + "; ".join(missing)


def _residual(lam, x, eta):
    return float(np.linalg.norm(lam.matvec(x) - eta) / np.linalg.norm(eta))


def test_accuracy_of_every_variant(runs):
    rows, bad = [], []
    for tag, res in runs["out"].items():
        for name in sf.NAMES:
            if name + "/x1" not in res:
                continue
            fx = runs["fixtures"][name]
            x_ref, x_lapack = runs["ref"][name]
            err = max(sf.component_errors(fx, res[name + "/x1"], x_ref))
            err_lapack = max(sf.component_errors(fx, x_lapack, x_ref))
            r = _residual(fx.lam, res[name + "/x1"], fx.eta)
            r2 = _residual(fx.lam, res[name + "/y"], np.random.default_rng(11).normal(size=fx.lam.n))
            rows.append("%-10s %-12s error %.2e (LAPACK %.2e) residual %.2e" % (tag, name, err, err_lapack, r))
            if not (err <= 1e-12 and r <= 1e-11 and r2 <= 1e-11):
                bad.append(rows[-1] + " second right-hand side residual %.2e" % r2)
    print("\n".join(rows))
    assert not bad, "\n".join(bad)


def test_forced_orderings_on_the_damped_pose_graphs(runs):
    """SPP_ORDERING=nd and =amd, otherwise chosen by a heuristic that these small graphs never tip"""
    import parity
    from slam_plus_plus_amd import synth
    from oracle import spp_oracle as orc
    for name in ("se2_small", "se3_small"):
        lam, eta = orc.assemble(synth.make(name), damping=50.0)
        x_true = parity.refined_solution(lam, eta)
        for o in ("nd", "amd"):
            res = runs["out"][o]
            x = res[name + "/x1"]
            err, r = parity.rel(x, x_true), _residual(lam, x, eta)
            print("%s SPP_ORDERING=%s: error %.2e residual %.2e, %d fronts on %d levels" % (
                name, o, err, r, res[name + "/front_h"].size, int(res[name + "/levels"])))
            assert err < 1e-10 and r <= 1e-11
            assert np.array_equal(x, res[name + "/x2"])
            assert np.array_equal(np.sort(res[name + "/order"]), np.arange(lam.nb))
        assert not np.array_equal(runs["out"]["nd"][name + "/order"], runs["out"]["amd"][name + "/order"]), "the switch changed nothing"


def test_solves_repeat_bit_for_bit(runs):
    for tag, res in runs["out"].items():
        for name in sf.NAMES:
            if name + "/x1" in res:
                assert np.array_equal(res[name + "/x1"], res[name + "/x2"]), (tag, name, "second solve")
                assert np.array_equal(res[name + "/x1"], res[name + "/x3"]), (tag, name, "after another right-hand side")


def test_split_launch_equals_the_default_bit_for_bit(runs):
    for name in sf.NAMES:
        assert np.array_equal(runs["out"]["split"][name + "/x1"], runs["out"]["default"][name + "/x1"]), name


def test_level_schedule_equals_the_default_up_to_192_rows(runs):
    """No class-4 front: both schedules run the same front_body with the children in list order, and the factor is the same
    bit for bit. The BACKWARD substitution is not the same code above 192 rows: the dependency-driven launch gives a front
    of h > 192 sixteen waves with eight columns in flight each (front_bwd_body<1024, 8>), the level schedule below the
    big fronts four waves with four (front_bwd_body<256, 4>), so the products right of a 64-pivot block are summed in
    another order (measured: the 192-wide clique of forest_a, h = 193, differs in the last bits).
    Hence bit for bit wherever every front has at most 192 rows -- per connected component in a forest, where a component
    is one front -- and the accuracy bound of test_accuracy_of_every_variant for the rest."""
    compared = 0
    for name in sf.NAMES:
        table = runs["out"]["default"]
        if np.any(table[name + "/front_cls"] == 4):
            continue
        fx = runs["fixtures"][name]
        x_levels, x_default = runs["out"]["levels"][name + "/x1"], runs["out"]["default"][name + "/x1"]
        if name in sf.FOREST_WIDTHS:
            for s in fx.comp_scalars:
                if s.size + 1 <= 192:     # a clique of width w is one front of w + 1 rows; the small tree is below anyway
                    compared += 1
                    assert np.array_equal(x_levels[s], x_default[s]), (name, s.size)
        elif table[name + "/front_h"].max() <= 192:
            compared += 1
            assert np.array_equal(x_levels, x_default), name
    assert compared >= 12, compared


def test_timed_out_launch_equals_the_level_schedule(runs):
    for name in sf.NAMES:
        assert np.array_equal(runs["out"]["timeout"][name + "/x1"], runs["out"]["levels"][name + "/x1"]), name


@pytest.mark.parametrize("variant", ["default", "noteams"])
def test_failure_paths(runs, variant):
    res = runs["out"][variant]
    for (name, width, what) in FAILURES:
        fx = runs["fixtures"][name]
        tag = "fail/%s:%d:%s" % (name, width, what)
        cls = {112: 2, 192: 3, 384: 4}[width]
        assert cls in res[name + "/front_cls"][res[name + "/front_w"] == width], "the broken clique is not of the class meant"
        assert np.array_equal(res[tag + "/rhs_after"], fx.eta), (tag, "the right-hand side was touched")
        err = max(sf.component_errors(fx, res[tag + "/x_after"], runs["ref"][name][0]))
        assert err <= 1e-12, (tag, err)
