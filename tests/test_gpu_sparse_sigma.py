"""GPU: spp_sparse_sigma_device -- the blocks of Sigma = Lambda^-1 on the stored pattern of Lambda by selected inversion
on the kept multifrontal factor (csrc/spp_sparse_sigma.hip), on the designed systems of tests/sparse_fixtures.py and, in
the default variant, the damped pose graphs se2_small / se3_small.

One child process (tests/sparse_sigma_child.py) per variant of the run-time switches, one after the other: the six of
tests/test_gpu_sparse_solve_again.py. This process asserts
  coverage       from the front tables of all children: every size class 0-4 as childless root, as parent and as child, and
                 every width of WIDTHS
  accuracy       per block column j, on its stored blocks: ||Sigma - ref||_F / ||ref||_F <= max(1e-10, 4 x the same error
                 of the EXISTING path), the existing path being sar.baseline_columns on vertex j's unit columns read at the
                 same rows and ref tests/sparse_sigma_ref.py: every block column of the components up to 700 scalars, the
                 sampled vertices of the larger ones. The library's new code is never the yardstick.
  full coverage  every stored block of every system against spp_sparse_solve_device on all n unit columns (the parent
                 commit's code): block-column relative difference <= 1e-10, the criterion's floor. A wrong rel, padded()
                 or transpose bit gives O(1).
  structure      diagonal blocks exactly symmetric and positive definite; sparse_block_diagonal()[v] against
                 sparse_marginals([v]) within the criterion (the summation orders differ: DESIGN.md section 29); every
                 double of a NaN-filled d_sigma overwritten, the NaN guards around it untouched
  bits           two calls; SPP_SPARSE_DAG=0 against the default where the factor has the same bits;
                 spp_factor_solve_device(eta) after the call against a ctx that never made it; spp_sparse_solve_device
                 before and after the call; SPARSE_FACTOR_KEPT 1 and FACTOR_KEPT 0 afterwards
  refusals       every refusal of the interface, each leaving d_sigma unwritten and the ctx usable.
The reference machinery is checked on the host by tests/test_sparse_sigma_ref_host.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import sparse_fixtures as sf
import sparse_sigma_ref as sgr
import sparse_solve_ref as ssr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "sparse_sigma_child.py")

FLOOR = 1e-10
E_BADARG, E_STATE, E_UNSUPPORTED = -1, -5, -6
NO_AMALG = {"SPP_AMALG_SMALL": "0", "SPP_AMALG_ZEROS": "0", "SPP_AMALG_ZEROS_SMALL": "0"}
# variant -> (switches beyond NO_AMALG, systems, refusals too)
VARIANTS = {
    "default": ({}, list(sf.NAMES) + list(ssr.POSE), True),
    "levels": ({"SPP_SPARSE_DAG": "0"}, sf.NAMES, False),
    "noteams": ({"SPP_SPARSE_TEAMS": "0"}, sf.NAMES, False),
    "mid128": ({"SPP_MID_FRONT_MAX": "128"}, sf.NAMES, False),
    "mid640": ({"SPP_MID_FRONT_MAX": "640"}, sf.NAMES, False),
}
FAILURE = ("forest_a", 112)      # FAILURES' class-2 case of tests/test_gpu_sparse_fronts.py: a negative pivot
WIDTHS = (1, 15, 16, 17, 48, 49, 112, 113, 191, 192, 304, 305, 384, 385, 624, 625, 1023, 1024)
ALL = list(sf.NAMES) + list(ssr.POSE)


def _child(tmp, tag, env_extra, args):
    out = tmp / (tag + ".npz")
    env = dict(os.environ)
    for k in list(env):
        if k.startswith("SPP_") and k != "SPP_LIB":
            del env[k]
    env.update(env_extra)
    r = subprocess.run([sys.executable, CHILD, str(tmp / "inputs.npz"), str(out)] + args, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, "%s: exit %d\n%s%s" % (tag, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return dict(np.load(out))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sparse_sigma")
    inputs = {}
    for name in ALL:
        lam, eta = ssr.problem(name)
        for k in ("dim", "col_ptr", "row_idx", "blk_off", "vals"):
            inputs["%s/%s" % (name, k)] = getattr(lam, k)
        inputs[name + "/eta"] = eta
        inputs[name + "/check"] = sgr.checked_vertices(name)
        inputs[name + "/sel"] = np.array(ssr.marginal_selection(name), dtype=np.int64)
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
        for name in ALL:
            if name + "/sigma" in res:
                yield tag, name, res


def test_every_variant_ran_its_systems(runs):
    seen = {}
    for tag, name, _ in _systems(runs):
        seen.setdefault(tag, []).append(name)
    assert seen == dict({tag: list(v[1]) for tag, v in VARIANTS.items()}, amalg=list(sf.TREE_NAMES)), seen
    assert max(ssr.problem(name)[0].n for name in sf.NAMES) == ssr.problem("forest_c")[0].n == 3366


def test_every_class_is_inverted_in_every_position(runs):
    cells = {}
    widths = set()
    for tag, name, res in _systems(runs):
        if name in ssr.POSE:
            continue
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


def test_accuracy_against_the_refined_inverse(runs):
    worst, bad = 0.0, []
    for tag, name, res in _systems(runs):
        lam = ssr.problem(name)[0]
        ref = sgr.reference_on_pattern(name)
        check = sgr.checked_vertices(name)
        err = sgr.column_errors(lam, res[name + "/sigma"], ref)[check]
        err_base = sgr.column_errors(lam, res[name + "/base"], ref)[check]
        bound = np.maximum(FLOOR, 4.0 * err_base)
        q = err / bound
        print("%s %s: %d block columns, largest error %.3e, of the existing path %.3e, largest quotient error / bound %.3e" % (
            tag, name, check.size, np.nanmax(err), np.nanmax(err_base), np.nanmax(q)))
        if not np.all(err <= bound):       # (fails on NaN too)
            bad.append((tag, name, float(np.nanmax(err)), int(np.sum(~(err <= bound)))))
        else:
            worst = max(worst, float(q.max()))
    print("largest quotient error / bound over every variant and system: %.3e" % worst)
    assert not bad, bad


def test_every_stored_block_against_the_solve_route(runs):
    bad = []
    for tag, name, res in _systems(runs):
        lam = ssr.problem(name)[0]
        sigma, solve = res[name + "/sigma"], res[name + "/solve"]
        assert not np.any(np.isnan(solve)), (tag, name, "the solve route left a stored double out")
        diff = sgr.column_errors(lam, sigma, solve)
        print("%s %s: %d block columns, largest relative difference from the solve route %.3e (bound %.0e)" % (
            tag, name, lam.nb, np.nanmax(diff), FLOOR))
        if not np.all(diff <= FLOOR):
            bad.append((tag, name, float(np.nanmax(diff)), int(np.sum(~(diff <= FLOOR)))))
    assert not bad, bad


def test_diagonal_blocks_symmetric_positive_definite_and_nothing_left_unwritten(runs):
    for tag, name, res in _systems(runs):
        lam = ssr.problem(name)[0]
        sigma = res[name + "/sigma"]
        assert not np.any(np.isnan(sigma)), (tag, name, "a double of d_sigma was not written")
        assert np.all(res[name + "/frames"]), (tag, name, "a NaN guard around d_sigma was written")
        assert int(res[name + "/n_diag"]) == lam.nb
        for v in range(lam.nb):
            d = int(lam.dim[v])
            p = int(lam.col_ptr[v + 1]) - 1
            blk = sigma[lam.blk_off[p]:lam.blk_off[p] + d * d].reshape((d, d), order="F")
            assert np.array_equal(blk, blk.T), (tag, name, v, "diagonal block not exactly symmetric")
            assert np.all(np.linalg.eigvalsh(blk) > 0), (tag, name, v, "diagonal block not positive definite")


def test_block_diagonal_agrees_with_the_marginals(runs):
    """sparse_block_diagonal()[v] is the stored diagonal block; against sparse_marginals([v]) it holds the criterion with
    the marginals as the existing path (the two sum in different orders: no bit identity)"""
    n = 0
    for tag, name, res in _systems(runs):
        lam = ssr.problem(name)[0]
        ref = sgr.reference_on_pattern(name)
        checked = set(int(v) for v in sgr.checked_vertices(name))
        for v in ssr.marginal_selection(name):
            d = int(lam.dim[v])
            p = int(lam.col_ptr[v + 1]) - 1
            at = slice(int(lam.blk_off[p]), int(lam.blk_off[p]) + d * d)
            diag, marg = res["%s/diag%d" % (name, v)], res["%s/marg%d" % (name, v)]
            assert np.array_equal(diag.ravel(order="F"), res[name + "/sigma_host"][at]), (tag, name, v)
            if v not in checked:
                continue
            r = ref[at].reshape((d, d), order="F")
            e_new, e_old = np.linalg.norm(diag - r) / np.linalg.norm(r), np.linalg.norm(marg - r) / np.linalg.norm(r)
            assert e_new <= max(FLOOR, 4.0 * e_old), (tag, name, v, e_new, e_old)
            n += 1
    assert n >= 4 * len(sf.NAMES), n


def test_two_calls_and_the_host_copy_agree_bit_for_bit(runs):
    for tag, name, res in _systems(runs):
        assert np.array_equal(res[name + "/sigma"], res[name + "/sigma2"]), (tag, name, "two calls differ")
        assert np.array_equal(res[name + "/sigma"], res[name + "/sigma_host"]), (tag, name, "Context.sparse_sigma differs")


def test_factor_and_solves_are_not_disturbed_and_the_flags_read_right(runs):
    for tag, name, res in _systems(runs):
        assert np.array_equal(res[name + "/X_before"], res[name + "/X_after"]), (tag, name, "spp_sparse_solve_device changed")
        assert np.array_equal(res[name + "/x_eta"], res[name + "/x_eta_after"]), (tag, name)
        assert np.array_equal(res[name + "/x_eta"], res[name + "/x_eta_fresh"]), (tag, name, "a ctx that never made the call differs")
        # SPARSE_FACTOR_KEPT after the factor, after the call, FACTOR_KEPT after the call, SPARSE_FACTOR_KEPT at the end
        assert list(res[name + "/kept"]) == [1, 1, 0, 1], (tag, name, res[name + "/kept"])


def test_level_schedule_equals_the_default_where_the_factor_does(runs):
    compared = 0
    for name in sf.NAMES:
        if np.any(runs["default"][name + "/front_cls"] == 4):
            continue
        compared += 1
        assert np.array_equal(runs["levels"][name + "/sigma"], runs["default"][name + "/sigma"]), name
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
            assert r[0] == expect[kind], (tag, r)
            assert r[1] == 1, (tag, "a refused call wrote to d_sigma")
            assert r[2] == 0, (tag, "SPARSE_FACTOR_KEPT")
    assert seen == {"state:before_analyze", "state:before_factor", "state:after_not_posdef", "state:after_analyze",
                    "state:after_dense_posv", "state:after_set_shard", "state:after_free_memory", "unsupported:sharded",
                    "unsupported:schur", "unsupported:schur_sparse", "unsupported:schur_mis"}, seen
    assert int(res["fail/status"]) == 1, "the designed negative pivot was not reported"
    r = res["refuse/badarg"]
    assert list(r) == [E_BADARG, E_BADARG, 1, 1], r
    for tag in ("after_first_refusals", "after_not_posdef", "after_badarg", "after_analyze", "after_dense_posv", "after_set_shard", "auto"):
        st, kept, frame, diff = res["usable/" + tag]
        assert st == 0 and kept == 1 and frame == 1 and diff <= FLOOR, (tag, res["usable/" + tag])
    assert int(res["auto/mode"]) == 1
    for tag in ("schur", "schur_sparse", "schur_mis"):
        st, resid = res["usable/" + tag]
        assert st == 0 and resid < 1e-10, (tag, resid)
