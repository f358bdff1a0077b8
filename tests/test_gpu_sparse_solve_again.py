"""GPU: spp_sparse_solve_device -- k further right-hand sides against the multifrontal factor a sparse solve left in the
fronts of its plan (csrc/spp_sparse_solve.hip), on the designed systems of tests/sparse_fixtures.py.

One child process per variant of the run-time switches (read once per process), one after the other; a child
(tests/sparse_solve_child.py) analyzes every system in MODE_SPARSE, runs the existing path on every column of
B = [eta, random, e of a leaf row, e of a separator row, random ...] (tests/sparse_solve_ref.py), then
spp_factor_solve_device(eta) and spp_sparse_solve_device with k = 1, 6, 17 (tree_hi: also 129, two passes). This process asserts
  coverage   from the front tables of all children: every size class 0-4 solved as childless root, as parent and as child,
             and both sides of every class boundary (the clique widths of the forests)
  accuracy   per column the residual ||Lambda x - b|| / ||b|| < 1e-11 and tests/parity.py's criterion with the EXISTING path
             as the reference backend: error against the refined column <= max(1e-10, 4 x the error of
             spp_factor_solve_device on that column). The library's new code is never the yardstick.
  bits       a column of a k-column solve is that column solved alone; a repeat; SPP_SPARSE_DAG=0 against the default where
             the factor has the same bits; the NaN frame around B; spp_factor_solve_device after a solve-again
  refusals   every refusal of the interface, each leaving B unwritten and the ctx usable.
The reference machinery is checked on the host by tests/test_sparse_solve_ref_host.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import solve_again_ref as sar
import sparse_fixtures as sf
import sparse_solve_ref as ssr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "sparse_solve_child.py")

RES_TOL = 1e-11
E_BADARG, E_STATE, E_UNSUPPORTED = -1, -5, -6
NO_AMALG = {"SPP_AMALG_SMALL": "0", "SPP_AMALG_ZEROS": "0", "SPP_AMALG_ZEROS_SMALL": "0"}
# variant -> (switches beyond NO_AMALG, fixtures, refusals too)
VARIANTS = {
    "default": ({}, sf.NAMES, True),
    "levels": ({"SPP_SPARSE_DAG": "0"}, sf.NAMES, False),
    "noteams": ({"SPP_SPARSE_TEAMS": "0"}, sf.NAMES, False),
    "mid128": ({"SPP_MID_FRONT_MAX": "128"}, sf.NAMES, False),
    "mid640": ({"SPP_MID_FRONT_MAX": "640"}, sf.NAMES, False),
}
FAILURE = ("forest_a", 112)      # FAILURES' class-2 case of tests/test_gpu_sparse_fronts.py: a negative pivot
WIDTHS = (1, 15, 16, 17, 48, 49, 112, 113, 191, 192, 304, 305, 384, 385, 624, 625, 1023, 1024)
ALONE = (0, 15, 16, 127, 128)


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
    tmp = tmp_path_factory.mktemp("sparse_solve_again")
    inputs = {}
    for name in sf.NAMES:
        lam, eta = ssr.problem(name)
        for k in ("dim", "col_ptr", "row_idx", "blk_off", "vals"):
            inputs["%s/%s" % (name, k)] = getattr(lam, k)
        inputs[name + "/eta"] = eta
        inputs[name + "/B"] = ssr.rhs_columns(name)
    fx = ssr.fixture(FAILURE[0])
    blocks = sf.clique_of_width(fx, FAILURE[1])["blocks"]
    v = int(blocks[blocks.size // 2])
    d = int(fx.lam.dim[v])
    off = int(fx.lam.blk_off[sf.diagonal_block(fx, v)]) + d * d - 1          # the block's last diagonal scalar
    inputs["fail_offset"] = np.int64(off)
    inputs["fail_value"] = np.float64(-abs(fx.lam.vals[off]))
    np.savez(tmp / "inputs.npz", **inputs)
    out = {}
    for tag, (switches, names, refuse) in VARIANTS.items():          # one after the other, never side by side
        out[tag] = _child(tmp, tag, dict(NO_AMALG, **switches), [",".join(names)] + (["refuse"] if refuse else []))
    out["amalg"] = _child(tmp, "amalg", {}, [",".join(sf.TREE_NAMES)])
    return out


def _systems(runs):
    for tag, res in runs.items():
        for name in sf.NAMES:
            if name + "/X1" in res:
                yield tag, name, res


def test_every_class_is_solved_in_every_position(runs):
    cells = {}
    widths = set()
    for tag, name, res in _systems(runs):
        t = {k: res["%s/front_%s" % (name, k)].astype(np.int64) for k in ("h", "w", "cls", "parent")}
        kid = t["parent"] >= 0
        n_children = np.bincount(t["parent"][kid], minlength=t["h"].size)
        for c in range(5):
            for what, hit in (("a childless root", (t["cls"] == c) & ~kid & (n_children == 0)),
                              ("a parent", (t["cls"] == c) & (n_children > 0)), ("a child", (t["cls"] == c) & kid)):
                key = "class %d as %s" % (c, what)
                cells[key] = cells.get(key, False) or bool(np.any(hit))
        widths |= set(int(w) for w in t["w"])
    missing = sorted(k for k, hit in cells.items() if not hit) + ["a front of width %d" % w for w in WIDTHS if w not in widths]
    assert not missing, "coverage cells without a front: " + "; ".join(missing)


def test_accuracy_of_every_variant(runs):
    worst, bad = 0.0, []
    for tag, name, res in _systems(runs):
        lam = ssr.problem(name)[0]
        B, Xref = ssr.rhs_columns(name), ssr.rhs_reference(name)
        e_base = sar.col_err(res[name + "/base"], Xref)
        for k in (1, 6, 17, 129):
            if "%s/X%d" % (name, k) not in res:
                continue
            X = res["%s/X%d" % (name, k)]
            r = np.array([np.linalg.norm(lam.matvec(X[:, j]) - B[:, j]) / np.linalg.norm(B[:, j]) for j in range(k)])
            print("%s %s k %d: largest residual %.3e (bound %.0e)" % (tag, name, k, r.max(), RES_TOL))
            if not np.all(r < RES_TOL):
                bad.append((tag, name, k, float(r.max())))
            worst = max(worst, sar.check_criterion(sar.col_err(X, Xref[:, :k]), e_base[:k], "%s %s k %d" % (tag, name, k)))
    assert all("tree_hi/X129" in res for res in runs.values()), "the two-pass solve did not run"
    print("largest quotient error / bound over every variant, system and k: %.3e" % worst)
    assert not bad, bad


def test_a_column_has_the_bits_of_that_column_solved_alone(runs):
    for tag, name, res in _systems(runs):
        kmax = ssr.rhs_columns(name).shape[1]
        X = res["%s/X%d" % (name, kmax)]
        assert np.array_equal(X, res[name + "/again"]), (tag, name, "two runs differ")
        for k in (1, 6, 17):
            assert np.array_equal(res["%s/X%d" % (name, k)], X[:, :k]), (tag, name, "the leading %d columns depend on k" % k)
        for j in ALONE:
            if j < kmax:
                assert np.array_equal(res["%s/alone%d" % (name, j)][:, 0], X[:, j]), (tag, name, "column %d depends on its neighbours or its position" % j)
    assert all("tree_hi/alone128" in res for tag, res in runs.items())


def test_nothing_outside_b_is_written(runs):
    for tag, name, res in _systems(runs):
        assert np.all(res[name + "/frames"]), (tag, name, "B was written outside its n rows / k columns")


def test_factor_solve_is_not_disturbed_and_the_flags_read_right(runs):
    for tag, name, res in _systems(runs):
        assert np.array_equal(res[name + "/x_eta"], res[name + "/x_eta_after"]), (tag, name)
        assert np.array_equal(res[name + "/x_eta"], res[name + "/x_eta_fresh"]), (tag, name, "a ctx that never solved again differs")
        # SPARSE_FACTOR_KEPT after analysis and the baseline solves (each keeps it), after the factor, after the solves; FACTOR_KEPT
        assert list(res[name + "/kept"]) == [1, 1, 1, 0], (tag, name, res[name + "/kept"])


def test_level_schedule_equals_the_default_where_the_factor_does(runs):
    """the solve on the kept factor is one code whatever schedule factored: where tests/test_gpu_sparse_fronts.py expects the
    two schedules to leave the same factor -- no class-4 front -- the solves have the same bits"""
    compared = 0
    for name in sf.NAMES:
        if np.any(runs["default"][name + "/front_cls"] == 4):
            continue
        compared += 1
        assert np.array_equal(runs["levels"][name + "/X17"], runs["default"][name + "/X17"]), name
    assert compared >= 3, compared


def test_refusals(runs):
    res = runs["default"]
    tags = [str(t) for t in res["refuse_tags"]]
    expect = {"state": E_STATE, "unsupported": E_UNSUPPORTED}
    seen = set()
    for tag in tags:
        r = res["refuse/" + tag]
        kind = tag.split(":")[0]
        if kind in expect:
            seen.add(tag)
            assert list(r[:2]) == [expect[kind]] * 2, (tag, r)
            assert r[2] == 1, (tag, "a refused call wrote to B")
            assert r[3] == 0, (tag, "SPARSE_FACTOR_KEPT")
    assert seen == {"state:before_analyze", "state:before_factor", "state:after_not_posdef", "state:after_analyze",
                    "state:after_dense_posv", "state:after_set_shard", "state:after_free_memory", "unsupported:sharded",
                    "unsupported:schur", "unsupported:schur_sparse", "unsupported:schur_mis"}, seen
    assert int(res["fail/status"]) == 1, "the designed negative pivot was not reported"
    r = res["refuse/dense_calls_on_sparse_ctx"]
    assert list(r) == [E_UNSUPPORTED, E_UNSUPPORTED, 1, 1], r
    r = res["refuse/badarg"]
    assert list(r[:-2]) == [E_BADARG] * 9 and r[-2] == 1 and r[-1] == 1, r
    for tag in ("after_first_refusals", "after_not_posdef", "after_badarg", "after_analyze", "after_dense_posv", "after_set_shard", "auto"):
        st, kept, frame, resid = res["usable/" + tag]
        assert st == 0 and kept == 1 and frame == 1 and resid < RES_TOL, (tag, res["usable/" + tag])
    assert int(res["auto/mode"]) == 1
    for tag in ("schur", "schur_sparse", "schur_mis"):
        st, resid = res["usable/" + tag]
        assert st == 0 and resid < 1e-10, (tag, resid)
