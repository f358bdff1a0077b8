"""Reference machinery of the solve-again tests (test infrastructure, numpy / scipy on the host only).

refined_columns(lam, B) is tests/parity.py's refined_solution column by column -- the same operations in the same order,
so the same bits (tests/test_solve_again_ref_host.py asserts it) -- with the sparse LU of Lambda computed once instead of
once per column (the LU is 0.4 s of the 0.5 s a column costs on the 36 000-row fixtures). covariance_ref assembles
E^T Lambda^-1 E from the refined unit columns. Everything is cached per fixture: the GPU tests share one reference."""
import numpy as np

import parity
import schur_fixtures_73 as fx73

K_MAX = 17
K_WIDE = {"edges32": 129, "loop32": 129}   # the fixtures that also run two passes of 128 columns (loop32: SCHEDULE_FIXTURES)
FIXTURES = ["tiny_shards", "edges32", "edges63", "edges63_long", "edges73", "edges73_aligned", "loop73"]
# tests/test_gpu_solve_again_schedules.py: the three dissected loops (6 x 3, 7 x 3, 3 x 2), the open chain in its natural
# order with unlisted tiles, and the pair-count spread
SCHEDULE_FIXTURES = ["loop63", "loop73", "loop32", "chain73", "edges63"]
COND_MAX = 1e6  # below it the 1e-10 floor of the parity criterion is above the reference's own error (cond * eps^2)

_CACHE = {}


def problem(name):
    if ("p", name) not in _CACHE:
        _CACHE[("p", name)] = fx73.make_any(name)
    return _CACHE[("p", name)]


class _Refiner:
    """parity.refined_solution with its LU and its longdouble image of Lambda kept"""

    def __init__(self, lam):
        import scipy.sparse.linalg as spla
        A = lam.to_scipy().tocsc()
        self.lu = spla.splu(A)
        C = A.tocoo()
        self.r, self.c, self.v = C.row, C.col, C.data.astype(np.longdouble)

    def solve(self, eta, iters=4):
        b = eta.astype(np.longdouble)
        x = self.lu.solve(eta).astype(np.longdouble)
        for _ in range(iters):
            res = b.copy()
            np.subtract.at(res, self.r, self.v * x[self.c])
            x = x + self.lu.solve(res.astype(np.float64)).astype(np.longdouble)
        return x.astype(np.float64)


def refiner(name):
    if ("lu", name) not in _CACHE:
        _CACHE[("lu", name)] = _Refiner(problem(name)[0])
    return _CACHE[("lu", name)]


def refined_columns(name, B):
    rf = refiner(name)
    return np.stack([rf.solve(np.ascontiguousarray(B[:, j])) for j in range(B.shape[1])], axis=1)


def vertex_rows(lam, vertices):
    return np.concatenate([np.arange(lam.base[v], lam.base[v + 1]) for v in vertices])


def unit_columns(lam, vertices):
    rows = vertex_rows(lam, vertices)
    E = np.zeros((lam.n, rows.size))
    E[rows, np.arange(rows.size)] = 1.0
    return E, rows


def covariance_ref(name, vertices):
    """(E^T Lambda^-1 E from refined unit-column solves, the refined columns themselves, the selected rows)"""
    lam = problem(name)[0]
    E, rows = unit_columns(lam, vertices)
    X = refined_columns(name, E)
    return X[rows], X, rows


def rhs_columns(name):
    """the right-hand sides of a fixture: [eta, random, e of a camera row, e of a landmark row, random ...], K_MAX columns
    (K_WIDE: more); the tests with fewer columns take the leading ones, so one reference serves them all"""
    if ("B", name) not in _CACHE:
        lam, eta = problem(name)
        k = K_WIDE.get(name, K_MAX)
        rng = np.random.default_rng(len(name) + 1000 * k)
        B = rng.standard_normal((lam.n, k))
        B[:, 0] = eta
        cams = np.flatnonzero(lam.dim == lam.dim.max())
        lms = np.flatnonzero(lam.dim == lam.dim.min())
        B[:, 2] = 0.0
        B[lam.base[cams[cams.size // 2]] + 1, 2] = 1.0
        B[:, 3] = 0.0
        B[lam.base[lms[lms.size // 3]] + int(lam.dim.min()) - 1, 3] = 1.0
        _CACHE[("B", name)] = B
    return _CACHE[("B", name)]


def rhs_reference(name):
    if ("X", name) not in _CACHE:
        _CACHE[("X", name)] = refined_columns(name, rhs_columns(name))
    return _CACHE[("X", name)]


def col_err(X, Xref):
    """per column ||x - x_ref|| / ||x_ref||"""
    return np.linalg.norm(X - Xref, axis=0) / np.linalg.norm(Xref, axis=0)


def condition(name):
    """cond_2 of the fixture's Lambda: dense for the small ones, else the extreme eigenvalues by Lanczos (the smallest by
    shift-invert on the LU the reference holds anyway)"""
    if ("cond", name) not in _CACHE:
        lam = problem(name)[0]
        if lam.n <= 2000:
            c = float(np.linalg.cond(lam.to_scipy().toarray()))
        else:
            import scipy.sparse.linalg as spla
            A = lam.to_scipy().tocsc()
            hi = spla.eigsh(A, k=1, which="LA", return_eigenvectors=False, tol=1e-6)[0]
            lu = refiner(name).lu
            op = spla.LinearOperator(A.shape, matvec=lu.solve, dtype=np.float64)
            lo = 1.0 / spla.eigsh(op, k=1, which="LA", return_eigenvectors=False, tol=1e-6)[0]
            c = float(hi / lo)
        _CACHE[("cond", name)] = c
    return _CACHE[("cond", name)]


def baseline_columns(ctx, d_vals, B):
    """the existing path on every column: one spp_factor_solve_device each (it is the yardstick's reference backend)"""
    from slam_plus_plus_amd import api
    d = api.DeviceArray(ctx, B.shape[0])
    out = np.empty_like(B)
    for j in range(B.shape[1]):
        d.upload(np.ascontiguousarray(B[:, j]))
        assert ctx.factor_solve_device(d_vals, d.ptr) == 0
        out[:, j] = d.download()
    d.free()
    return out


def check_criterion(err, err_base, what):
    """tests/parity.py's criterion with the existing path as the reference backend: per column
    err <= max(1e-10, 4 err(existing path)); returns the largest quotient err / that bound"""
    bound = np.maximum(1e-10, 4.0 * err_base)
    q = err / bound
    print("%s: largest error %.3e, of the existing path %.3e, largest quotient error / bound %.3e" % (
        what, err.max(), err_base.max(), q.max()))
    assert np.all(err <= bound), (what, err, bound)   # (fails on NaN too)
    return float(q.max())
