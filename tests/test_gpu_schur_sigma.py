"""GPU: spp_schur_sigma_device -- the blocks of Sigma = Lambda^-1 on the stored pattern of Lambda from the kept dense Schur
factor (csrc/spp_schur_sigma.hip on csrc/spp_dense_potri.h), on the fixtures of tests/schur_sigma_ref.py:

  tiny_shards      24 reduced rows: one partial tile          chain73          7 x 3, 644 rows: five tiles and a sliver, open
  loop32, loop63   3 x 2 / 6 x 3 dissected loops (900 / 1800)                   chain with unlisted tiles
  edges63_long     6 x 3: pair-count spread, 256- and 257-track, unobserved and degree-1 landmarks, A blocks incl. a camera
                   that observes nothing                      edges73_aligned  the same coverage with 7-wide cameras
  ba_interleaved   interleaved numbering: observation blocks stored landmark row first

One child process (tests/schur_sigma_child.py) per variant of the run-time switches, one after the other: the default on
all seven, and SPP_DENSE_TAIL=0, SPP_TAIL_MASK=0, SPP_SCHUR_CAM_ORDER=0, SPP_SACC_FACTORED=0 (the plan keeps cinv) on
loop63 and chain73. The parent asserts.

  accuracy   per block column, ||sigma - ref||_F / ||ref||_F on its stored blocks <= max(1e-10, 4 x the same of the existing
             path: spp_solve_device on that vertex's unit columns, read at the same rows); ref tests/schur_sigma_ref.py.
             Every block column up to n = 11 000; on the edges fixtures all cameras and the landmark selection.
  coverage   tiny_shards, chain73, loop32, loop63: every stored block also against spp_solve_device on all n unit columns
  structure  NaN-filled d_sigma wholly overwritten, guards untouched, diagonal blocks exactly symmetric and positive
             definite, schur_block_diagonal()[v] the stored block bit for bit and within the criterion of marginals([v])
  bits       two calls; spp_solve_device before / after; a following spp_factor_solve_device against a ctx that never
             made the call; FACTOR_KEPT = 1; the variants whose factor has the default's bits (DESIGN.md section 31:
             SPP_TAIL_MASK=0 on both, SPP_SCHUR_CAM_ORDER=0 on chain73) have the default's sigma
  refusals   in this process, at the places tests/test_gpu_solve_again.py visits

The reference machinery is checked on the host by tests/test_schur_sigma_ref_host.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import schur_sigma_ref as ssg
import solve_again_ref as sar
import sparse_sigma_ref as sgr
from slam_plus_plus_amd import api

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "schur_sigma_child.py")

FLOOR = 1e-10
E_BADARG, E_STATE, E_UNSUPPORTED = -1, -5, -6
SCHEDULED = ["loop63", "chain73"]
VARIANTS = {
    "default": ({}, ssg.FIXTURES),
    "notail": ({"SPP_DENSE_TAIL": "0"}, SCHEDULED),
    "nomask": ({"SPP_TAIL_MASK": "0"}, SCHEDULED),
    "natural": ({"SPP_SCHUR_CAM_ORDER": "0"}, SCHEDULED),
    "cinv": ({"SPP_SACC_FACTORED": "0"}, SCHEDULED),
}
SAME_BITS = [("nomask", "loop63"), ("nomask", "chain73"), ("natural", "chain73")]   # the factor has the default's bits


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


def _marginal_vertices(name):
    """five vertices: the first, middle and last camera, the first and the last landmark"""
    P = ssg.parts(name)
    return np.array([P.cams[0], P.cams[P.cams.size // 2], P.cams[-1], P.lms[0], P.lms[-1]], dtype=np.int64)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("schur_sigma")
    inputs = {}
    for name in ssg.FIXTURES:
        lam, eta = ssg.problem(name)
        for k in ("dim", "col_ptr", "row_idx", "blk_off", "vals"):
            inputs["%s/%s" % (name, k)] = getattr(lam, k)
        inputs[name + "/eta"] = eta
        inputs[name + "/check"] = ssg.checked_vertices(name)
        inputs[name + "/sel"] = _marginal_vertices(name)
    np.savez(tmp / "inputs.npz", **inputs)
    out = {}
    for tag, (switches, names) in VARIANTS.items():          # one after the other, never side by side
        out[tag] = _child(tmp, tag, switches, [",".join(names)])
    return out


def _systems(runs):
    for tag, (_, names) in VARIANTS.items():
        for name in names:
            yield tag, name, runs[tag]


def test_every_variant_ran_its_systems_under_its_switches(runs):
    for tag, (switches, names) in VARIANTS.items():
        assert sorted(runs[tag]["env"].tolist()) == sorted("%s=%s" % kv for kv in switches.items()), tag
        for name in names:
            assert name + "/sigma" in runs[tag], (tag, name)
    for name in ssg.FIXTURES:
        lam = ssg.problem(name)[0]
        all_checked = ssg.checked_vertices(name).size == lam.nb
        assert all_checked == (not name.startswith("edges")), name
    assert all(ssg.problem(name)[0].n <= ssg.N_ALL for name in ssg.FULL)


def test_accuracy_against_the_reference(runs):
    worst, bad = 0.0, []
    for tag, name, res in _systems(runs):
        lam = ssg.problem(name)[0]
        ref = ssg.reference(name)
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


def test_every_stored_block_against_the_solve_route(runs):
    for tag, name, res in _systems(runs):
        if name not in ssg.FULL:
            continue
        lam = ssg.problem(name)[0]
        ref = ssg.reference(name)
        route = res[name + "/base"]
        assert not np.any(np.isnan(route)), (tag, name, "the solve route did not cover every stored double")
        err = sgr.column_errors(lam, res[name + "/sigma"], route)
        bound = np.maximum(FLOOR, 4.0 * sgr.column_errors(lam, route, ref))
        print("%s %s: every stored block against spp_solve_device on %d unit columns: largest difference %.3e" % (
            tag, name, lam.n, err.max()))
        assert np.all(err <= bound), (tag, name, float(err.max()))


def test_structure(runs):
    for tag, name, res in _systems(runs):
        lam = ssg.problem(name)[0]
        sigma = res[name + "/sigma"]
        assert sigma.shape == (lam.nvals,) and not np.any(np.isnan(sigma)), (tag, name, "a double of d_sigma was not written")
        assert res[name + "/frames"].all(), (tag, name, "a guard was written")
        assert np.array_equal(res[name + "/sigma_host"], sigma), (tag, name, "Context.schur_sigma differs")
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
        assert np.array_equal(res[name + "/diag_all"], np.concatenate(stored)), (tag, name, "schur_block_diagonal is not the stored blocks")
        err, err_m = [], []
        ref = ssg.reference(name)
        for v in _marginal_vertices(name):
            p = int(lam.col_ptr[v + 1]) - 1
            d = int(lam.dim[v])
            sl = slice(int(lam.blk_off[p]), int(lam.blk_off[p]) + d * d)
            D = res["%s/diag%d" % (name, v)]
            assert np.array_equal(D.ravel(order="F"), sigma[sl]), (tag, name, v, "schur_block_diagonal is not the stored block")
            R = ref[sl].reshape((d, d), order="F")
            err.append(np.linalg.norm(D - R) / np.linalg.norm(R))
            err_m.append(np.linalg.norm(res["%s/marg%d" % (name, v)] - R) / np.linalg.norm(R))
        sar.check_criterion(np.array(err), np.array(err_m), "%s %s diagonal blocks against marginals([v])" % (tag, name))


def test_bits(runs):
    for tag, name, res in _systems(runs):
        assert np.array_equal(res[name + "/sigma"], res[name + "/sigma2"]), (tag, name, "two calls differ")
        assert np.array_equal(res[name + "/X_before"], res[name + "/X_after"]), (tag, name, "spp_solve_device changed")
        assert np.array_equal(res[name + "/x_eta"], res[name + "/x_eta_after"]), (tag, name)
        assert np.array_equal(res[name + "/x_eta_after"], res[name + "/x_eta_fresh"]), (tag, name, "the next factor differs")
        assert res[name + "/kept"].tolist() == [1, 1, 1], (tag, name)
    for tag, name in SAME_BITS:
        assert np.array_equal(runs[tag][name + "/x_eta"], runs["default"][name + "/x_eta"]), (tag, name, "DESIGN.md section 31")
        assert np.array_equal(runs[tag][name + "/sigma"], runs["default"][name + "/sigma"]), (tag, name)


# ---- refusals: each leaves d_sigma unwritten and the ctx usable -----------------------------------------------------
def _factor(c, dv, eta):
    dr = api.DeviceArray.from_host(c, eta)
    st = c.factor_solve_device(dv.ptr, dr.ptr)
    x = dr.download()
    dr.free()
    return st, x


def _refused(c, dv, nvals, code, kept=0):
    dS = api.DeviceArray.from_host(c, np.ones(max(1, nvals)))
    assert c.lib.spp_schur_sigma_device(c.h, dv.ptr, dS.ptr) == code
    assert np.array_equal(dS.download(), np.ones(max(1, nvals))), "a refused call wrote to d_sigma"
    out = ctypes.c_int64(-1)
    assert c.lib.spp_get_info(c.h, api.INFO["FACTOR_KEPT"], ctypes.byref(out)) == 0 and out.value == kept
    dS.free()


def _usable(c, name, lam, eta, dv):
    st, _ = _factor(c, dv, eta)
    assert st == 0 and c.info("FACTOR_KEPT") == 1
    sigma = c.schur_sigma(dv.ptr)
    ref = ssg.reference(name)
    assert np.all(sgr.column_errors(lam, sigma, ref) <= 1e-9) and c.info("FACTOR_KEPT") == 1


def test_refused_without_a_kept_factor_and_the_ctx_stays_usable():
    name = "edges73_aligned"
    lam, eta = ssg.problem(name)
    nv = lam.nvals
    c = api.Context(0)
    dv = api.DeviceArray.from_host(c, lam.vals)
    _refused(c, dv, nv, E_STATE)                         # before any analysis
    c.analyze(lam, api.MODE_SCHUR)
    _refused(c, dv, nv, E_STATE)                         # before any factor
    _usable(c, name, lam, eta, dv)
    vals = lam.vals.copy()                               # after a failed pivot (tests/test_gpu_solve_again.py's construction)
    lm = int(np.flatnonzero(lam.dim == 3)[17])
    p = lam.col_ptr[lm + 1] - 1
    C = vals[lam.blk_off[p]:lam.blk_off[p] + 9].reshape(3, 3)
    ev = np.linalg.eigvalsh(C)
    C -= 0.5 * (ev[0] + ev[1]) * np.eye(3)
    dbad = api.DeviceArray.from_host(c, vals)
    assert _factor(c, dbad, eta)[0] == api.SPP_NOT_POSDEF
    _refused(c, dv, nv, E_STATE)
    dbad.free()
    _usable(c, name, lam, eta, dv)
    c.analyze(lam, api.MODE_SCHUR)                       # after analyze
    _refused(c, dv, nv, E_STATE)
    _usable(c, name, lam, eta, dv)
    A = np.eye(5) * 3.0                                  # after spp_dense_posv
    dA, db = api.DeviceArray.from_host(c, A.ravel()), api.DeviceArray.from_host(c, np.ones(5))
    assert c._check(c.lib.spp_dense_posv(c.h, dA.ptr, 5, 5, db.ptr)) == 0
    _refused(c, dv, nv, E_STATE)
    _usable(c, name, lam, eta, dv)
    dZ = api.DeviceArray(c, 25)                          # after spp_dense_potri
    dA.upload(A.ravel())
    assert c.dense_potri(dA.ptr, 5, 5, dZ.ptr, 5) == 0
    dA.free(); db.free(); dZ.free()
    _refused(c, dv, nv, E_STATE)
    _usable(c, name, lam, eta, dv)
    dS = api.DeviceArray(c, c.schur_buffer_size())       # after the split form, on a caller's buffer too
    dr = api.DeviceArray.from_host(c, eta)
    c.schur_form(dv.ptr, dr.ptr, dS.ptr)
    _refused(c, dv, nv, E_STATE)
    assert c.schur_finish(dv.ptr, dS.ptr, dr.ptr) == 0
    _refused(c, dv, nv, E_STATE)
    dS.free(); dr.free()
    _usable(c, name, lam, eta, dv)
    c.set_shard(0, 1)                                    # after spp_set_shard
    _refused(c, dv, nv, E_STATE)
    c.analyze(lam, api.MODE_SCHUR)
    _usable(c, name, lam, eta, dv)
    assert c.lib.spp_free_memory(c.h) == 0               # after spp_free_memory (the workspace goes with it)
    _refused(c, dv, nv, E_STATE)
    c.analyze(lam, api.MODE_SCHUR)
    _usable(c, name, lam, eta, dv)
    dv.free()
    c.close()


@pytest.mark.parametrize("name,mode", [("edges73_aligned", api.MODE_SPARSE), ("edges73_aligned", api.MODE_SCHUR_SPARSE),
                                       ("mis33", api.MODE_SCHUR_MIS)])
def test_unsupported_modes_are_refused(name, mode):
    lam, eta = sar.problem(name)
    c = api.Context(0)
    c.analyze(lam, mode)
    dv = api.DeviceArray.from_host(c, lam.vals)
    assert _factor(c, dv, eta)[0] == 0
    _refused(c, dv, lam.nvals, E_UNSUPPORTED)
    st, x = _factor(c, dv, eta)                          # the ctx goes on solving in its own mode
    assert st == 0 and np.linalg.norm(lam.matvec(x) - eta) / np.linalg.norm(eta) < 1e-10
    dv.free()
    c.close()


def test_a_sharded_ctx_is_refused():
    name = "tiny_shards"
    lam, eta = ssg.problem(name)
    c = api.Context(0)
    c.set_shard(0, 2)
    c.analyze(lam, api.MODE_SCHUR)
    dv = api.DeviceArray.from_host(c, lam.vals)
    _refused(c, dv, lam.nvals, E_UNSUPPORTED)
    c.set_shard(0, 1)
    c.analyze(lam, api.MODE_SCHUR)
    _usable(c, name, lam, eta, dv)
    dv.free()
    c.close()


def test_the_sparse_call_stays_unsupported_and_null_pointers_leave_the_factor_kept():
    name = "tiny_shards"
    lam, eta = ssg.problem(name)
    c = api.Context(0)
    c.analyze(lam, api.MODE_SCHUR)
    dv = api.DeviceArray.from_host(c, lam.vals)
    assert _factor(c, dv, eta)[0] == 0
    dS = api.DeviceArray.from_host(c, np.ones(lam.nvals))
    lib, h = c.lib, c.h
    assert lib.spp_sparse_sigma_device(h, dS.ptr) == E_UNSUPPORTED
    assert lib.spp_schur_sigma_device(h, None, dS.ptr) == E_BADARG
    assert lib.spp_schur_sigma_device(h, dv.ptr, None) == E_BADARG
    assert lib.spp_schur_sigma_device(None, dv.ptr, dS.ptr) == E_BADARG
    assert np.array_equal(dS.download(), np.ones(lam.nvals)) and c.info("FACTOR_KEPT") == 1
    dS.free()
    sigma = c.schur_sigma(dv.ptr)
    assert np.all(sgr.column_errors(lam, sigma, ssg.reference(name)) <= 1e-9)
    dv.free()
    c.close()
