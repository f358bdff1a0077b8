"""GPU: the streamed dense factor with a step order (spp_dense_posv_ordered; the Schur plan hands one over under a dissected
camera order): a tile applies the steps its mask selects in the order of a list instead of k ascending.
Matrices: two arcs (bands that do not see each other) and separator rows coupled to both, diagonally dominant like those
of tests/test_gpu_dense_tilemask.py.

The identity gives the bits of spp_dense_posv_masked. The depth order (api.tail_step_order_host) sums in another order:
bit-identical repeats, the residual bound of the dense tests (1e-12), the componentwise backward bound of a Cholesky
factorization, which holds for ANY order of the sums (Higham, Accuracy and Stability of Numerical Algorithms, theorem
10.3: |A - R^T R| <= gamma_(n+1) |R^T| |R|), the factor of numpy.linalg.cholesky to the accuracy the identity order
reaches on the same matrix, exact zeros outside the filled pattern, a failed pivot reported from arc B and from the
separator. The Schur stage on the 300-camera loop of tests/test_gpu_cam_order.py with SPP_TAIL_STEP_ORDER 1 and 0 in child
processes: both within the longdouble reference's bound, each bit-reproducible."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from slam_plus_plus_amd import api

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
NB = 128
EPS = np.finfo(np.float64).eps
E_BADARG = -1   # SPP_E_BADARG of include/spp_hip.h
_CACHE = {}


def _system(ta, tb, ts, n, seed, factor=True):
    """arcs of ta and tb tile rows (bands of half-width 100 that do not see each other), ts separator tile rows coupled to
    every row; n <= 128 (ta + tb + ts) cuts the last tile. Returns A, b, the tile mask words, numpy's factor"""
    key = (ta, tb, ts, n, seed, factor)
    if key in _CACHE:
        return _CACHE[key]
    tr = ta + tb + ts
    assert NB * (tr - 1) < n <= NB * tr
    r = np.arange(n)
    part = np.where(r < NB * ta, 0, np.where(r < NB * (ta + tb), 1, 2))
    E = ((part[:, None] == part[None, :]) & (np.abs(r[:, None] - r[None, :]) <= 100)) | (part[None, :] == 2) | (part[:, None] == 2)
    rng = np.random.default_rng(seed)
    A = np.triu(np.where(E, rng.standard_normal((n, n)), 0.0), 1)
    A = A + A.T
    A[np.diag_indices(n)] = np.abs(A).sum(axis=1) + 1.0 + rng.random(n)
    b = rng.standard_normal(n)
    pad = np.zeros((NB * tr, NB * tr), bool)
    pad[:n, :n] = E
    M = np.triu(pad.reshape(tr, NB, tr, NB).any(axis=(1, 3)))
    assert not M[:ta, ta:ta + tb].any(), "a tile couples the two arcs"
    words = np.array([sum(1 << int(j) for j in np.flatnonzero(row)) for row in M], np.uint64)
    _CACHE[key] = (A, b, words, np.linalg.cholesky(A).T if factor else None)
    return _CACHE[key]


def _posv(ctx, A, b, words, order=None):
    n = A.shape[0]
    dA = api.DeviceArray.from_host(ctx, np.asfortranarray(A).reshape(-1, order="F"))
    db = api.DeviceArray.from_host(ctx, b)
    w = np.ascontiguousarray(words, dtype=np.uint64)
    if order is None:
        st = ctx._check(ctx.lib.spp_dense_posv_masked(ctx.h, dA.ptr, n, n, db.ptr, w.ctypes.data, w.size))
    else:
        o = np.ascontiguousarray(order, dtype=np.int32)
        assert o.size == w.size
        st = ctx._check(ctx.lib.spp_dense_posv_ordered(ctx.h, dA.ptr, n, n, db.ptr, w.ctypes.data, w.size, o.ctypes.data))
    streamed = ctx.info("DENSE_STREAMED")
    R = np.triu(dA.download().reshape((n, n), order="F"))
    x = db.download()
    dA.free()
    db.free()
    return st, R, x, streamed


def _filled(words, n):
    tr = len(words)
    F = np.zeros((tr, n // NB + 1), bool)
    for i, w in enumerate(words):
        F[i, [j for j in range(F.shape[1]) if (int(w) >> j) & 1]] = True
    F[np.arange(tr), np.arange(tr)] = True
    F[:, n // NB] = True
    F &= np.triu(np.ones(F.shape, bool))
    for k in range(tr):
        r = np.flatnonzero(F[k, k + 1:]) + k + 1
        for a in r[r < tr]:
            F[a, r[r >= a]] = True
    return F


# (2, 3, 2) cut to 890: the smallest two arcs of different lengths with two separator rows, a partial last tile, the right-hand
# side in the last tile row's column; (4, 5, 16) at 3200: 136 tiles in the separator triangle, the right-hand side in a
# tile column of its own
SHAPES = [(2, 3, 2, 890), (4, 5, 16, 3200)]


@pytest.mark.parametrize("ta,tb,ts,n", SHAPES)
def test_identity_equals_the_masked_call_and_the_depth_order_factors_as_well(hip_ctx, ta, tb, ts, n):
    A, b, words, Rref = _system(ta, tb, ts, n, n)
    tr = ta + tb + ts
    st0, R0, x0, s0 = _posv(hip_ctx, A, b, words)
    assert st0 == 0 and s0 == tr, (st0, s0)          # the whole factorization was the streamed launch
    st1, R1, x1, s1 = _posv(hip_ctx, A, b, words, np.arange(tr))
    assert st1 == 0 and s1 == tr
    assert np.array_equal(R1, R0) and np.array_equal(x1, x0), "the identity order does not give the masked call's bits"
    so = api.tail_step_order_host(n, words)
    m = min(ta, tb)
    assert np.array_equal(so[:2 * m], np.stack([np.arange(m), ta + np.arange(m)], 1).ravel()), so
    assert np.array_equal(so[ta + tb:], np.arange(ta + tb, tr)), so
    runs = [_posv(hip_ctx, A, b, words, so) for _ in range(2)]
    for st, R, x, s in runs:
        assert st == 0 and s == tr
    R, x = runs[0][1], runs[0][2]
    assert np.array_equal(R, runs[1][1]) and np.array_equal(x, runs[1][2]), "not bit-reproducible"
    res = np.abs(A @ x - b).max() / np.abs(b).max()
    gamma = (n + 1) * EPS / (1.0 - (n + 1) * EPS)
    num, den = np.abs(A - R.T @ R), np.abs(R).T @ np.abs(R)
    assert not num[den == 0].any()
    back = (num[den > 0] / den[den > 0]).max() / gamma
    err_id, err = np.abs(R0 - Rref).max(), np.abs(R - Rref).max()
    print("n %d, order %s: residual %.2e, backward error / bound %.3f, |R - chol| %.2e (identity order %.2e), R differs in %d entries"
          % (n, so.tolist(), res, back, err, err_id, int((R != R0).sum())))
    assert res < 1e-12
    assert back <= 1.0
    # numpy's factor, to the accuracy the identity order reaches: the two runs round the same sums in another association
    # -- two samples of one error distribution, a factor of 4 between their maxima covers that; a lost, doubled or
    # misplaced update shows at 1e-3 and above
    assert err <= 4.0 * max(err_id, EPS * np.abs(Rref).max()), (err, err_id)
    F = _filled(words, n)
    for i in range(tr):
        for j in range(i, tr):
            if not F[i, j]:
                assert not R[NB * i:NB * (i + 1), NB * j:NB * (j + 1)].any(), (i, j)
    assert not F[:ta, ta:ta + tb].any()


def test_the_order_must_be_a_permutation(hip_ctx):
    A, b, words, _ = _system(2, 3, 2, 890, 890)
    lib, n = hip_ctx.lib, 890
    dA = api.DeviceArray.from_host(hip_ctx, np.asfortranarray(A).reshape(-1, order="F"))
    db = api.DeviceArray.from_host(hip_ctx, b)
    for bad in ([0, 1, 2, 3, 4, 5, 5], [0, 1, 2, 3, 4, 5, 7], [-1, 1, 2, 3, 4, 5, 6]):
        o = np.array(bad, np.int32)
        assert lib.spp_dense_posv_ordered(hip_ctx.h, dA.ptr, n, n, db.ptr, words.ctypes.data, 7, o.ctypes.data) == E_BADARG
    o = np.arange(7, dtype=np.int32)
    assert lib.spp_dense_posv_ordered(hip_ctx.h, dA.ptr, n, n, db.ptr, words.ctypes.data, 7, None) == E_BADARG
    assert lib.spp_dense_posv_ordered(hip_ctx.h, dA.ptr, n, n, db.ptr, None, 0, o.ctypes.data) == E_BADARG
    assert np.array_equal(db.download(), b), "a rejected call touched the right-hand side"
    dA.free()
    db.free()


@pytest.mark.parametrize("ta,tb,ts,n", SHAPES)
@pytest.mark.parametrize("where", ["arc B", "separator"])
def test_a_failed_pivot_is_reported_and_the_repaired_matrix_factors(hip_ctx, ta, tb, ts, n, where):
    A, b, words, _ = _system(ta, tb, ts, n, n)
    A = A.copy()
    bad = NB * ta + NB * tb // 2 + 5 if where == "arc B" else NB * (ta + tb) + (n - NB * (ta + tb)) // 2
    keep = A[bad, bad]
    A[bad, bad] = -1.0
    so = api.tail_step_order_host(n, words)
    st, _, _, _ = _posv(hip_ctx, A, b, words, so)
    assert st == api.SPP_NOT_POSDEF, st
    A[bad, bad] = keep
    st, R, x, s = _posv(hip_ctx, A, b, words, so)
    assert st == 0 and s == ta + tb + ts
    assert np.abs(A @ x - b).max() / np.abs(b).max() < 1e-12


# ---- the Schur stage: the plan's step order on and off -------------------------------------------------------------------
CHILD = r"""
import sys, json, hashlib
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import test_gpu_cam_order as t
from slam_plus_plus_amd import api
lam, eta = t.system("loop")
c = api.Context(0)
c.analyze(lam, api.MODE_SCHUR)
dv, dr = api.DeviceArray.from_host(c, lam.vals), api.DeviceArray(c, lam.n)
xs = []
for _ in range(2):
    dr.upload(eta)
    assert c.factor_solve_device(dv.ptr, dr.ptr) == 0
    xs.append(dr.download())
np.save(sys.argv[1], xs[0])
print(json.dumps({"sha": [hashlib.sha256(x.tobytes()).hexdigest() for x in xs], "order": c.ordering(lam.nb)[:c.info("N_POSES")].tolist(),
                  "streamed": c.info("DENSE_STREAMED"), "so": api.schur_step_order_host(lam).tolist()}))
"""


def _solve_in_child(env, out):
    e = {k: v for k, v in os.environ.items() if k not in ("SPP_TAIL_STEP_ORDER", "SPP_TAIL_MASK")}
    e.update(env, SPP_VERBOSE="1")
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, TESTS), out], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    d = json.loads(r.stdout.strip().split("\n")[-1])
    d["ordered"] = "in the caller's step order" in r.stderr
    assert d["sha"][0] == d["sha"][1], "x not bit-reproducible with %s" % env
    return d, np.load(out)


def test_schur_stage_with_the_step_order_on_and_off(tmp_path):
    import schur_ref
    import test_gpu_cam_order as t
    lam, eta = t.system("loop")
    on, x_on = _solve_in_child({"SPP_TAIL_STEP_ORDER": "1"}, str(tmp_path / "on.npy"))
    off, x_off = _solve_in_child({"SPP_TAIL_STEP_ORDER": "0"}, str(tmp_path / "off.npy"))
    nomask, x_nomask = _solve_in_child({"SPP_TAIL_MASK": "0"}, str(tmp_path / "nomask.npy"))
    ident = list(range(15))
    assert on["order"] == off["order"] != list(range(t.NC)), "the camera order does not depend on the step order's switch"
    assert on["streamed"] == 15 and off["streamed"] == 15
    assert on["ordered"] and on["so"] != ident and sorted(on["so"]) == ident
    assert not off["ordered"] and off["so"] == ident
    # SPP_TAIL_MASK = 0 sees the same step order and gives the same bits (that switch changes scheduling alone)
    assert nomask["ordered"] and nomask["so"] == on["so"] and nomask["sha"] == on["sha"]
    P = t._ref_in_order(lam, eta, np.asarray(on["order"]))
    for tag, x in (("on", x_on), ("off", x_off)):
        print("step order %s: landmark / pose part, error / bound: %s" % (tag, schur_ref.check_solution(P, lam, eta, x)))
    print("on against off: relative difference %.3e" % (np.linalg.norm(x_on - x_off) / np.linalg.norm(x_off)))


# ---- the leading rows of a run too large to be seated whole (SPP_TAIL_EARLY_LEAD): another table, the same bits ---------------
# (4, 5, 16): at 256 resident workgroups its lagging run (rows 15 ..) is seated whole, with the switch on or off; (7, 8, 16) at
# 3968: the 16 separator rows lag, 152 tiles against 128 -- their leading rows are seated with the switch on, nothing with it off
LEAD_CHILD = r"""
import sys, json, hashlib
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import test_gpu_dense_step_order as t
from slam_plus_plus_amd import api
out = {}
ctx = api.Context(0, 0)
for ta, tb, ts, n in json.loads(sys.argv[1]):
    A, b, words, _ = t._system(ta, tb, ts, n, n, factor=False)
    so = api.tail_step_order_host(n, words)
    st, R, x, s = t._posv(ctx, A, b, words, so)
    assert st == 0 and s == ta + tb + ts, (st, s)
    out[str(n)] = [hashlib.sha256(R.tobytes()).hexdigest(), hashlib.sha256(x.tobytes()).hexdigest()]
ctx.close()
print("RESULT " + json.dumps(out))
"""
LEAD_SHAPES = [(4, 5, 16, 3200), (7, 8, 16, 3968)]


def _lead_child(switch):
    import re
    env = {k: v for k, v in os.environ.items() if k not in ("SPP_TAIL_EARLY_LEAD", "SPP_TAIL_EARLY", "SPP_TAIL_MASK")}
    env.update(SPP_TAIL_EARLY_LEAD=switch, SPP_VERBOSE="1")
    r = subprocess.run([sys.executable, "-c", LEAD_CHILD % (ROOT, TESTS), json.dumps(LEAD_SHAPES)], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    sha = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    tables = re.findall(r"streamed tail: (\d+) x (\d+) tiles, (\d+) listed, (\d+) resident; (\d+) tiles of rows (\d+)\.\. seated first "
                        r"\(whole rows resident (\d+), live demand (\d+)\)", r.stderr)
    return sha, [tuple(int(v) for v in t) for t in tables]


def test_leading_rows_change_the_table_and_not_the_bits():
    on, tab_on = _lead_child("1")
    off, tab_off = _lead_child("0")
    assert on == off, "SPP_TAIL_EARLY_LEAD changed R or x"
    assert len(tab_on) == len(tab_off) == len(LEAD_SHAPES), (tab_on, tab_off)
    for (ta, tb, ts, n), t_on, t_off in zip(LEAD_SHAPES, tab_on, tab_off):
        _, _, words, _ = _system(ta, tb, ts, n, n, factor=False)
        words = np.array([sum(1 << int(j) for j in np.flatnonzero(row)) for row in _filled(words, n)], np.uint64)   # (the probe takes the FILLED mask)
        resident = t_on[3]
        assert resident > 0 and t_off[3] == resident
        for early, got in ((3, t_on), (1, t_off)):   # the host probe's table for the device's resident count
            tiles, info = api.tail_order_host(n, words, resident=resident, early=early)
            assert got == (ta + tb + ts, n // NB + 1, len(tiles), resident, info["n_early"], info["r_star"], info["rows_resident"],
                           info["live_demand"]), (n, early, got, info)
        print("n %d, %d resident: seated first with the switch on %d tiles of rows %d.., off %d tiles of rows %d.." % (
            n, resident, t_on[4], t_on[5], t_off[4], t_off[5]))
        if resident == 256 and n == 3968:
            assert t_off[4] == 0 and 0 < t_on[4] <= 128 and t_on[5] == 15, (t_on, t_off)
