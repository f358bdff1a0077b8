"""GPU: the kept factor of a SPARSE reduced system (MODE_SCHUR_SPARSE) --
spp_schur_sparse_solve_device, spp_schur_sparse_marginals_device, spp_schur_sparse_sigma_device -- on the fixtures of
tests/schur_sigma_ref.py and cliques63 of tests/schur_sparse_again_ref.py (fronts of classes 3 and 4, each as parent and
as child), all analyzed in MODE_SCHUR_SPARSE explicitly.

One child process (tests/schur_sparse_again_child.py) per variant of the run-time switches, one after the other: the default
on all eight; SPP_SPARSE_DAG=0, SPP_SPARSE_TEAMS=0, SPP_MID_FRONT_MAX=128, SPP_MID_FRONT_MAX=640, SPP_SACC_FACTORED=0 (the
plan keeps cinv) on loop63, chain73 and cliques63. The parent asserts.

  coverage   from Context.sparse_fronts() of the default variant: classes 0 - 4 occur, classes 3 and 4 each as parent and child
  accuracy   the project's criterion, error <= max(1e-10, 4 x the error of the existing path against the same refined
             reference), per column or per block column. Which existing path backs which check:
               solves (k = 1, 6, 17; loop32: 129) and marginals -- spp_factor_solve_device in MODE_SCHUR_SPARSE, one call
                   per column (sar.baseline_columns' route), reference sar.refined_columns / sar.covariance_ref;
               sigma, every block column up to n = 11 000, on the edges fixtures all cameras and the landmark selection --
                   spp_solve_device on the unit columns in a second ctx analyzed in MODE_SCHUR (thousands of columns: one
                   factorization each is out of reach), reference schur_sigma_ref.reference;
               every stored block against spp_schur_sparse_solve_device on all n unit columns on tiny_shards, chain73,
                   loop32, loop63 and cliques63 -- bound from that route's own error against the reference.
  bits       column j of a k-column solve is that column solved alone (positions 0, 15, 16, 127, 128); a repeat; sigma
             twice; a solve before / after sigma; a following spp_factor_solve_device against a ctx that never made the calls
  structure  NaN-filled d_sigma wholly overwritten, guards and the slack rows of d_B (ldb > n) untouched, diagonal blocks
             exactly symmetric and positive definite, schur_sparse_block_diagonal()[v] the stored block bit for bit
  state      SCHUR_SPARSE_FACTOR_KEPT 1 after SPP_OK and through the new calls, FACTOR_KEPT and SPARSE_FACTOR_KEPT 0
             throughout; refusals in this process, at the places tests/test_gpu_solve_again.py visits

The reference machinery of cliques63 is checked on the host by tests/test_schur_sparse_again_ref_host.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import schur_sigma_ref as ssg
import schur_sparse_again_ref as ssa
import solve_again_ref as sar
import sparse_sigma_ref as sgr
from slam_plus_plus_amd import api

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "schur_sparse_again_child.py")

FLOOR = 1e-10
E_BADARG, E_STATE, E_UNSUPPORTED = -1, -5, -6
ALONE = (0, 15, 16, 127, 128)
VARIANTS = {
    "default": ({}, ssa.FIXTURES),
    "nodag": ({"SPP_SPARSE_DAG": "0"}, ssa.SCHEDULED),
    "noteams": ({"SPP_SPARSE_TEAMS": "0"}, ssa.SCHEDULED),
    "mid128": ({"SPP_MID_FRONT_MAX": "128"}, ssa.SCHEDULED),
    "mid640": ({"SPP_MID_FRONT_MAX": "640"}, ssa.SCHEDULED),
    "cinv": ({"SPP_SACC_FACTORED": "0"}, ssa.SCHEDULED),
}


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
    tmp = tmp_path_factory.mktemp("schur_sparse_again")
    inputs = {"full": np.array(ssa.FULL)}
    for name in ssa.FIXTURES:
        lam, eta = ssa.problem(name)
        for k in ("dim", "col_ptr", "row_idx", "blk_off", "vals"):
            inputs["%s/%s" % (name, k)] = getattr(lam, k)
        inputs[name + "/eta"] = eta
        inputs[name + "/B"] = sar.rhs_columns(name)
        inputs[name + "/check"] = ssg.checked_vertices(name)
        inputs[name + "/sel"] = ssa.marginal_vertices(name)
    np.savez(tmp / "inputs.npz", **inputs)
    out = {}
    for tag, (switches, names) in VARIANTS.items():          # one after the other, never side by side
        out[tag] = _child(tmp, tag, switches, [",".join(names)])
    return out


def _systems(runs):
    for tag, (_, names) in VARIANTS.items():
        for name in names:
            yield tag, name, runs[tag]


def _widths(name):
    k = sar.rhs_columns(name).shape[1]
    return (1, 6, 17) + ((k,) if k > 17 else ())


def test_every_variant_ran_its_systems_under_its_switches(runs):
    for tag, (switches, names) in VARIANTS.items():
        assert sorted(runs[tag]["env"].tolist()) == sorted("%s=%s" % kv for kv in switches.items()), tag
        for name in names:
            assert name + "/sigma" in runs[tag], (tag, name)
    for name in ssa.FIXTURES:
        lam = ssa.problem(name)[0]
        assert (ssg.checked_vertices(name).size == lam.nb) == (not name.startswith("edges")), name
    assert all(ssa.problem(name)[0].n <= ssg.N_ALL for name in ssa.FULL)
    assert sar.rhs_columns("loop32").shape[1] == 129 and "loop32/alone128" in runs["default"]


def test_front_classes_0_to_4_occur_and_3_and_4_as_parent_and_as_child(runs):
    res = runs["default"]
    seen, as_parent, as_child = set(), set(), set()
    for name in ssa.FIXTURES:
        cls, parent = res[name + "/front_cls"], res[name + "/front_parent"]
        print("%s: %d fronts, per class %s" % (name, cls.size, np.bincount(cls, minlength=5).tolist()))
        seen |= set(cls.tolist())
        has = parent >= 0
        as_child |= set(cls[has].tolist())
        as_parent |= set(cls[parent[has]].tolist())
    assert seen == {0, 1, 2, 3, 4}, seen
    assert {3, 4} <= as_parent and {3, 4} <= as_child, (as_parent, as_child)
    # the designed fixture alone gives the two large classes in both roles
    cls, parent = res[ssa.NEW + "/front_cls"], res[ssa.NEW + "/front_parent"]
    has = parent >= 0
    assert {3, 4} <= set(cls[has].tolist()) and {3, 4} <= set(cls[parent[has]].tolist())
    # the switch moves the threshold between the two
    assert 3 not in set(runs["mid128"][ssa.NEW + "/front_cls"].tolist())
    assert 4 not in set(runs["mid640"][ssa.NEW + "/front_cls"].tolist())


def test_solves_against_the_refined_reference(runs):
    for tag, name, res in _systems(runs):
        Xref = sar.rhs_reference(name)
        err_base = sar.col_err(res[name + "/base_B"], Xref)
        for k in _widths(name):
            X = res["%s/X%d" % (name, k)]
            assert X.shape == (Xref.shape[0], k)
            sar.check_criterion(sar.col_err(X, Xref[:, :k]), err_base[:k], "%s %s k = %d" % (tag, name, k))


def test_marginals_against_the_refined_reference(runs):
    for tag, name, res in _systems(runs):
        sel = ssa.marginal_vertices(name)
        cov_ref = sar.covariance_ref(name, sel)[0]
        cov = res[name + "/marg"]
        assert cov.shape == cov_ref.shape and np.array_equal(cov, cov.T), (tag, name, "the covariance is not exactly symmetric")
        np.linalg.cholesky(cov)
        sar.check_criterion(sar.col_err(cov, cov_ref), sar.col_err(res[name + "/base_marg"], cov_ref),
                            "%s %s marginals of %s" % (tag, name, sel.tolist()))


def test_sigma_against_the_reference(runs):
    worst, bad = 0.0, []
    for tag, name, res in _systems(runs):
        lam = ssa.problem(name)[0]
        ref = ssa.reference(name)
        check = ssg.checked_vertices(name)
        err = sgr.column_errors(lam, res[name + "/sigma"], ref)[check]
        err_base = sgr.column_errors(lam, res[name + "/base"], np.where(np.isnan(res[name + "/base"]), np.nan, ref))[check]
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


def test_every_stored_block_against_the_new_solve_route(runs):
    for tag, name, res in _systems(runs):
        if name not in ssa.FULL:
            continue
        lam = ssa.problem(name)[0]
        ref = ssa.reference(name)
        route = res[name + "/route"]
        assert not np.any(np.isnan(route)), (tag, name, "the solve route did not cover every stored double")
        err = sgr.column_errors(lam, res[name + "/sigma"], route)
        bound = np.maximum(FLOOR, 4.0 * sgr.column_errors(lam, route, ref))
        print("%s %s: every stored block against spp_schur_sparse_solve_device on %d unit columns: largest difference %.3e" % (
            tag, name, lam.n, err.max()))
        assert np.all(err <= bound), (tag, name, float(err.max()))


def test_structure(runs):
    for tag, name, res in _systems(runs):
        lam = ssa.problem(name)[0]
        sigma = res[name + "/sigma"]
        assert sigma.shape == (lam.nvals,) and not np.any(np.isnan(sigma)), (tag, name, "a double of d_sigma was not written")
        assert res[name + "/frames"].all(), (tag, name, "a guard, a slack row or a spare column was written")
        assert np.array_equal(res[name + "/sigma_host"], sigma), (tag, name, "Context.schur_sparse_sigma differs")
        assert int(res[name + "/n_diag"]) == lam.nb
        p = lam.col_ptr[1:] - 1                    # (upper incl. diagonal, rows ascending: the diagonal block closes its column)
        assert np.array_equal(lam.row_idx[p], np.arange(lam.nb))
        stored = []
        for d in np.unique(lam.dim):               # every vertex of a width as one (N, d, d) stack
            at = lam.blk_off[p[lam.dim == d]]
            D = sigma[at[:, None] + np.arange(d * d)[None, :]].reshape(-1, d, d).transpose(0, 2, 1)
            assert np.array_equal(D, D.transpose(0, 2, 1)), (tag, name, d, "a diagonal block is not exactly symmetric")
            np.linalg.cholesky(D)                  # (raises unless every block of the stack is positive definite)
            assert np.all(np.linalg.eigvalsh(D)[:, 0] > 0), (tag, name, d)
        for v in range(lam.nb):
            d = int(lam.dim[v])
            stored.append(sigma[int(lam.blk_off[p[v]]):int(lam.blk_off[p[v]]) + d * d])
        assert np.array_equal(res[name + "/diag_all"], np.concatenate(stored)), (tag, name, "schur_sparse_block_diagonal is not the stored blocks")


def test_bits(runs):
    for tag, name, res in _systems(runs):
        widths = _widths(name)
        kmax = widths[-1]
        Xk = res["%s/X%d" % (name, kmax)]
        assert np.array_equal(res[name + "/again"], Xk), (tag, name, "two solves differ, or ldb matters")
        for k in widths:
            assert np.array_equal(res["%s/X%d" % (name, k)], Xk[:, :k]), (tag, name, k, "a column depends on how many the call carries")
        for j in ALONE:
            if j < kmax:
                assert np.array_equal(res["%s/alone%d" % (name, j)][:, 0], Xk[:, j]), (
                    tag, name, "column %d depends on its neighbours or its position" % j)
        assert np.array_equal(res[name + "/sigma"], res[name + "/sigma2"]), (tag, name, "two sigma calls differ")
        assert np.array_equal(res[name + "/X_before"], res[name + "/X_after"]), (tag, name, "the solve changed over a sigma call")
        assert np.array_equal(res[name + "/x_eta"], res[name + "/x_eta_after"]), (tag, name)
        assert np.array_equal(res[name + "/x_eta_after"], res[name + "/x_eta_fresh"]), (tag, name, "the next factor differs")


def test_the_info_words(runs):
    for tag, name, res in _systems(runs):
        kept = res[name + "/kept"]     # after analyze | after the last factor | after solves + marginals | after sigma | at the end | after the next factor
        assert kept[:, 0].tolist() == [0, 1, 1, 1, 1, 1], (tag, name, kept)
        assert not kept[:, 1:].any(), (tag, name, "FACTOR_KEPT or SPARSE_FACTOR_KEPT was set in this mode")


# ---- state and refusals: each leaves its output unwritten and the ctx usable ------------------------------------------
def _factor(c, dv, eta):
    dr = api.DeviceArray.from_host(c, eta)
    st = c.factor_solve_device(dv.ptr, dr.ptr)
    x = dr.download()
    dr.free()
    return st, x


def _word(c, name):
    out = ctypes.c_int64(-1)
    assert c.lib.spp_get_info(c.h, api.INFO[name], ctypes.byref(out)) == 0
    return out.value


def _refused(c, dv, lam, code, kept=0):
    """all three calls answer `code`, write nothing, and leave the three words (kept, 0, 0) -- or what the mode's own is"""
    n, nv = lam.n, max(1, lam.nvals)
    before = [_word(c, w) for w in ("SCHUR_SPARSE_FACTOR_KEPT", "FACTOR_KEPT", "SPARSE_FACTOR_KEPT")]
    assert before[0] == kept
    dS = api.DeviceArray.from_host(c, np.ones(nv))
    dB = api.DeviceArray.from_host(c, np.ones(2 * n))
    dC = api.DeviceArray.from_host(c, np.ones(64))
    v = np.array([0], dtype=np.int64)
    lib, h = c.lib, c.h
    assert lib.spp_schur_sparse_sigma_device(h, dv.ptr, dS.ptr) == code
    assert lib.spp_schur_sparse_solve_device(h, dv.ptr, dB.ptr, n, 2) == code
    assert lib.spp_schur_sparse_marginals_device(h, dv.ptr, 1, v.ctypes.data, dC.ptr) == code
    assert np.array_equal(dS.download(), np.ones(nv)), "a refused call wrote to d_sigma"
    assert np.array_equal(dB.download(), np.ones(2 * n)), "a refused call wrote to d_B"
    assert np.array_equal(dC.download(), np.ones(64)), "a refused call wrote to d_cov"
    assert [_word(c, w) for w in ("SCHUR_SPARSE_FACTOR_KEPT", "FACTOR_KEPT", "SPARSE_FACTOR_KEPT")] == before
    for d in (dS, dB, dC):
        d.free()


def _usable(c, name, lam, eta, dv):
    st, x = _factor(c, dv, eta)
    assert st == 0 and c.info("SCHUR_SPARSE_FACTOR_KEPT") == 1 and c.info("FACTOR_KEPT") == 0 and c.info("SPARSE_FACTOR_KEPT") == 0
    assert np.linalg.norm(lam.matvec(x) - eta) / np.linalg.norm(eta) < 1e-10
    sigma = c.schur_sparse_sigma(dv.ptr)
    assert np.all(sgr.column_errors(lam, sigma, ssa.reference(name)) <= 1e-9) and c.info("SCHUR_SPARSE_FACTOR_KEPT") == 1
    dB = api.DeviceArray.from_host(c, eta)
    assert c.schur_sparse_solve_device(dv.ptr, dB.ptr, 1) == 0
    xs = dB.download()
    dB.free()
    assert np.linalg.norm(xs - x) / np.linalg.norm(x) < 1e-9 and c.info("SCHUR_SPARSE_FACTOR_KEPT") == 1


def test_refused_without_a_kept_factor_and_the_ctx_stays_usable():
    name = "chain73"
    lam, eta = ssa.problem(name)
    mode = api.MODE_SCHUR_SPARSE
    c = api.Context(0)
    dv = api.DeviceArray.from_host(c, lam.vals)
    _refused(c, dv, lam, E_STATE)                        # before any analysis (the word needs none)
    c.analyze(lam, mode)
    _refused(c, dv, lam, E_STATE)                        # before any factor
    _usable(c, name, lam, eta, dv)
    # after a failed pivot: a negated camera block, the construction tests/test_gpu_schur_sparse.py uses in this mode (the
    # status of a sparse reduced system is its factor's alone, and a landmark block with a negative eigenvalue only adds
    # to S: the dense mode's construction with a landmark block need not fail here)
    vals = lam.vals.copy()
    cam = int(np.flatnonzero(lam.dim == 7)[3])
    p = lam.col_ptr[cam + 1] - 1
    vals[lam.blk_off[p]:lam.blk_off[p] + 49] *= -1.0
    dbad = api.DeviceArray.from_host(c, vals)
    assert _factor(c, dbad, eta)[0] == api.SPP_NOT_POSDEF
    _refused(c, dv, lam, E_STATE)
    dbad.free()
    _usable(c, name, lam, eta, dv)
    c.analyze(lam, mode)                                 # after analyze
    _refused(c, dv, lam, E_STATE)
    _usable(c, name, lam, eta, dv)
    A = np.eye(5) * 3.0                                  # after spp_dense_posv
    dA, db = api.DeviceArray.from_host(c, A.ravel()), api.DeviceArray.from_host(c, np.ones(5))
    assert c._check(c.lib.spp_dense_posv(c.h, dA.ptr, 5, 5, db.ptr)) == 0
    _refused(c, dv, lam, E_STATE)
    _usable(c, name, lam, eta, dv)
    dZ = api.DeviceArray(c, 25)                          # after spp_dense_potri
    dA.upload(A.ravel())
    assert c.dense_potri(dA.ptr, 5, 5, dZ.ptr, 5) == 0
    dA.free(); db.free(); dZ.free()
    _refused(c, dv, lam, E_STATE)
    _usable(c, name, lam, eta, dv)
    dS = api.DeviceArray(c, c.schur_buffer_size())       # after the split form, on a caller's buffer too
    dr = api.DeviceArray.from_host(c, eta)
    c.schur_form(dv.ptr, dr.ptr, dS.ptr)
    _refused(c, dv, lam, E_STATE)
    assert c.schur_finish(dv.ptr, dS.ptr, dr.ptr) == 0
    _refused(c, dv, lam, E_STATE)
    dS.free(); dr.free()
    _usable(c, name, lam, eta, dv)
    c.set_shard(0, 1)                                    # after spp_set_shard
    _refused(c, dv, lam, E_STATE)
    c.analyze(lam, mode)
    _usable(c, name, lam, eta, dv)
    assert c.lib.spp_free_memory(c.h) == 0               # after spp_free_memory (the workspaces go with it)
    _refused(c, dv, lam, E_STATE)
    c.analyze(lam, mode)
    _usable(c, name, lam, eta, dv)
    dv.free()
    c.close()


@pytest.mark.parametrize("name,mode", [("edges73_aligned", api.MODE_SPARSE), ("edges73_aligned", api.MODE_SCHUR),
                                       ("mis33", api.MODE_SCHUR_MIS)])
def test_unsupported_modes_are_refused(name, mode):
    lam, eta = sar.problem(name)
    c = api.Context(0)
    c.analyze(lam, mode)
    dv = api.DeviceArray.from_host(c, lam.vals)
    assert _factor(c, dv, eta)[0] == 0
    _refused(c, dv, lam, E_UNSUPPORTED)
    st, x = _factor(c, dv, eta)                          # the ctx goes on solving in its own mode
    assert st == 0 and np.linalg.norm(lam.matvec(x) - eta) / np.linalg.norm(eta) < 1e-10
    assert _word(c, "SCHUR_SPARSE_FACTOR_KEPT") == 0
    dv.free()
    c.close()


def test_a_sharded_ctx_is_refused():
    name = "tiny_shards"
    lam, eta = ssa.problem(name)
    c = api.Context(0)
    c.set_shard(0, 2)
    c.analyze(lam, api.MODE_SCHUR_SPARSE)
    dv = api.DeviceArray.from_host(c, lam.vals)
    _refused(c, dv, lam, E_UNSUPPORTED)
    c.set_shard(0, 1)
    c.analyze(lam, api.MODE_SCHUR_SPARSE)
    _usable(c, name, lam, eta, dv)
    dv.free()
    c.close()


def test_the_six_older_calls_stay_refused_and_bad_arguments_leave_the_factor_kept():
    name = "tiny_shards"
    lam, eta = ssa.problem(name)
    n, nv = lam.n, lam.nvals
    c = api.Context(0)
    c.analyze(lam, api.MODE_SCHUR_SPARSE)
    dv = api.DeviceArray.from_host(c, lam.vals)
    assert _factor(c, dv, eta)[0] == 0
    dS = api.DeviceArray.from_host(c, np.ones(nv))
    dB = api.DeviceArray.from_host(c, np.ones(n))
    dC = api.DeviceArray.from_host(c, np.ones(64))
    v = np.array([0], dtype=np.int64)
    twice = np.array([1, 1], dtype=np.int64)
    far = np.array([lam.nb], dtype=np.int64)
    lib, h = c.lib, c.h
    assert lib.spp_solve_device(h, dv.ptr, dB.ptr, n, 1) == E_UNSUPPORTED
    assert lib.spp_marginals_device(h, dv.ptr, 1, v.ctypes.data, dC.ptr) == E_UNSUPPORTED
    assert lib.spp_schur_sigma_device(h, dv.ptr, dS.ptr) == E_UNSUPPORTED
    assert lib.spp_sparse_solve_device(h, dB.ptr, n, 1) == E_UNSUPPORTED
    assert lib.spp_sparse_marginals_device(h, 1, v.ctypes.data, dC.ptr) == E_UNSUPPORTED
    assert lib.spp_sparse_sigma_device(h, dS.ptr) == E_UNSUPPORTED
    assert c.info("SCHUR_SPARSE_FACTOR_KEPT") == 1       # (the six keep it)
    assert lib.spp_schur_sparse_sigma_device(h, None, dS.ptr) == E_BADARG
    assert lib.spp_schur_sparse_sigma_device(h, dv.ptr, None) == E_BADARG
    assert lib.spp_schur_sparse_sigma_device(None, dv.ptr, dS.ptr) == E_BADARG
    assert lib.spp_schur_sparse_solve_device(h, None, dB.ptr, n, 1) == E_BADARG
    assert lib.spp_schur_sparse_solve_device(h, dv.ptr, None, n, 1) == E_BADARG
    assert lib.spp_schur_sparse_solve_device(h, dv.ptr, dB.ptr, n, 0) == E_BADARG
    assert lib.spp_schur_sparse_solve_device(h, dv.ptr, dB.ptr, n - 1, 1) == E_BADARG
    assert lib.spp_schur_sparse_marginals_device(h, dv.ptr, 0, v.ctypes.data, dC.ptr) == E_BADARG
    assert lib.spp_schur_sparse_marginals_device(h, dv.ptr, 1, None, dC.ptr) == E_BADARG
    assert lib.spp_schur_sparse_marginals_device(h, dv.ptr, 1, v.ctypes.data, None) == E_BADARG
    assert lib.spp_schur_sparse_marginals_device(h, dv.ptr, 2, twice.ctypes.data, dC.ptr) == E_BADARG
    assert lib.spp_schur_sparse_marginals_device(h, dv.ptr, 1, far.ctypes.data, dC.ptr) == E_BADARG
    assert np.array_equal(dS.download(), np.ones(nv)) and np.array_equal(dB.download(), np.ones(n))
    assert np.array_equal(dC.download(), np.ones(64))
    assert c.info("SCHUR_SPARSE_FACTOR_KEPT") == 1 and c.info("FACTOR_KEPT") == 0 and c.info("SPARSE_FACTOR_KEPT") == 0
    for d in (dS, dB, dC):
        d.free()
    sigma = c.schur_sparse_sigma(dv.ptr)
    assert np.all(sgr.column_errors(lam, sigma, ssa.reference(name)) <= 1e-9)
    dv.free()
    c.close()
