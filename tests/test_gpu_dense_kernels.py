"""The dense factor's pieces against plain fp64 / extended-precision references, at the shapes where they go wrong:
the upper-only trailing update the factorization makes (and what it must leave alone), the partial factorization of a
big sparse front (identity padding after the pivots, a contribution block below them), the accuracy of the backward
substitution on ill-conditioned systems, state carried from one call to the next, and a failed pivot in the per-step
part of a factorization."""
import numpy as np
import pytest
import scipy.linalg as sla

from slam_plus_plus_amd import api

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


# ---- the upper-only trailing update (dense_gemm_tn_sub(..., upper_only = true)) ------------------------------------
# upper_only: 128 x 128 tiles of C on or above the diagonal band are written (whole), the rest are skipped. t128 = (tile
# rows x tile columns) / 2 + 1 selects the kernel: >= 50 (and k % 32 == 0) the mixed-granularity kernel, otherwise the
# 64 x 64 kernel -- or, for k % 32 != 0, the 128 x 128 kernel from 192 on.
@pytest.mark.parametrize("m,n,k", [
    (128, 128, 128), (129, 130, 128), (192, 320, 128), (127, 127, 128),            # m = 0, 1, 64, 127 mod 128
    (1151, 1151, 128), (1151, 1152, 128),                                            # t128 = 41: 64 x 64 tiles
    (1217, 1217, 128), (1217, 1218, 128), (1280, 1408, 128), (1279, 1407, 128),      # t128 >= 50: mixed granularity
    (2624, 2752, 128), (2561, 2562, 128),                                            # mixed, more tiles than slots
    (2432, 2433, 48), (2561, 2561, 48), (2687, 2815, 16),                            # k % 32 != 0: t128 191 / 221 / 232
])
def test_gemm_tn_sub_upper_matches_numpy_and_leaves_the_rest(hip_ctx, m, n, k):
    rng = np.random.default_rng(1000 * m + n + k)
    lda, ldb, ldc = k + 2, k + 4, m + 5
    A = rng.standard_normal((k, m))
    B = rng.standard_normal((k, n))
    C = rng.standard_normal((m, n))
    want = C - A.T @ B
    Af = np.zeros((lda, m), order="F"); Af[:k] = A
    Bf = np.zeros((ldb, n), order="F"); Bf[:k] = B
    Cf = np.full((ldc, n), np.nan, order="F")
    Cf[:m] = C
    i, j = np.indices((m, n))
    below = i > j
    skipped = (i // 128) > (j // 128)           # tiles strictly below the diagonal band: never written
    Cf[:m][skipped] = np.nan
    # sentinels in rows m .. ldc-1 and in the skipped tiles, compared bit for bit afterwards: in even columns a NaN with a
    # payload (were it read into a written tile, the upper part would turn NaN), in odd columns finite values (a write
    # changes them; a NaN would come back from C - A^T B with its payload intact and hide the write)
    sentinel = np.frombuffer(np.uint64(0x7ff8dead0000beef).tobytes(), dtype=np.float64)[0]
    odd = np.zeros((ldc, n), dtype=bool); odd[:, 1::2] = True
    nan = np.isnan(Cf)
    Cf[nan & ~odd] = sentinel
    Cf[nan & odd] = 3.0 + rng.random(int((nan & odd).sum()))
    before = Cf.copy()
    dA = api.DeviceArray.from_host(hip_ctx, Af.ravel(order="F"))
    dB = api.DeviceArray.from_host(hip_ctx, Bf.ravel(order="F"))
    dC = api.DeviceArray.from_host(hip_ctx, Cf.ravel(order="F"))
    hip_ctx._check(hip_ctx.lib.spp_dense_gemm_tn_sub_upper(hip_ctx.h, m, n, k, dA.ptr, lda, dB.ptr, ldb, dC.ptr, ldc))
    out = dC.download().reshape((ldc, n), order="F")
    for d in (dA, dB, dC):
        d.free()
    got = out[:m]
    up = ~below
    err = np.abs(got[up] - want[up]).max() / max(1.0, np.abs(want).max())
    assert err < 1e-13, err
    # bit-identical: the ld padding rows and every entry of the skipped tiles
    assert out[m:].view(np.uint64).tobytes() == before[m:].view(np.uint64).tobytes(), "rows >= m were written"
    assert np.array_equal(got[skipped].view(np.uint64), before[:m][skipped].view(np.uint64)), "a tile below the diagonal was written"
    # strictly-lower entries inside the diagonal tiles belong to tiles the update writes whole (the factorization never
    # reads them): each is either untouched or the exact update
    inner = below & ~skipped
    untouched = got[inner].view(np.uint64) == before[:m][inner].view(np.uint64)
    updated = np.abs(got[inner] - want[inner]) <= 1e-13 * max(1.0, np.abs(want).max())
    assert np.all(untouched | updated)


# ---- partial factorization of a big front (spp_sparse.hip: identity padding after the w pivots) ---------------------
def _front_matrix(h, seed, rank=256):
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((h, min(rank, h)))
    A = G @ G.T / min(rank, h)
    A[np.diag_indices(h)] += 1.0 + rng.random(h)
    return A


def _front_factor(ctx, A, w, expect=api.SPP_OK):
    h = A.shape[0]
    pad = (w + 127) // 128 * 128 - w
    hp = h + pad
    ldp = (hp + 1) & ~1
    ld = h + 3
    F = np.full((ld, h), 7.0, order="F")
    F[:h] = A
    dF = api.DeviceArray.from_host(ctx, F.ravel(order="F"))
    dI = api.DeviceArray(ctx, ldp * hp)
    st = ctx._check(ctx.lib.spp_dense_front_factor(ctx.h, dF.ptr, ld, w, h, dI.ptr))
    out = dF.download().reshape((ld, h), order="F")
    img = dI.download().reshape((ldp, hp), order="F")[:hp]
    dF.free(); dI.free()
    assert st == expect
    assert np.all(out[h:] == 7.0), "rows >= h of the caller's array were written"
    return out[:h], img, pad


def _front_reference(A, w):
    R11 = np.linalg.cholesky(A[:w, :w]).T
    R12 = sla.solve_triangular(R11, A[:w, w:], trans="T", lower=False)
    S = A[w:, w:] - R12.T @ R12
    return R11, R12, S


@pytest.mark.parametrize("w,c", [(64, 300), (97, 400), (100, 700), (129, 0), (129, 1), (129, 2900), (300, 0), (300, 130), (640, 1), (640, 257),
                                 (640, 2900), (700, 0), (700, 1), (700, 1000), (700, 2900)])
def test_front_factor_matches_lapack(hip_ctx, w, c):
    """w pivots, c rows of contribution block (w < 128: the first diagonal block is part padding; w = 97: a single valid
    pivot in the last 16-wide panel the diagonal-block kernel factors). c = 2900 puts more than 2560 trailing rows behind the first steps: those
    take the two-stream schedule (flags from 4 steps on: w = 640, 700; events below: w = 129)."""
    h = w + c
    A = _front_matrix(h, 17 * w + c)
    out, img, pad = _front_factor(hip_ctx, A, w)
    R11, R12, S = _front_reference(A, w)
    amax = np.abs(A).max()
    G11 = np.triu(out[:w, :w])
    assert np.abs(G11.T @ G11 - A[:w, :w]).max() / amax < 1e-13
    assert np.abs(G11 - R11).max() / np.abs(R11).max() < 1e-11
    if c:
        assert np.abs(out[:w, w:] - R12).max() / np.abs(R12).max() < 1e-11
        iu = np.triu_indices(c)
        assert np.abs(out[w:, w:][iu] - S[iu]).max() / amax < 1e-13
    # the identity padding comes back as identity: pivots [w, w + pad), their rows right of the diagonal and their columns
    # above it
    if pad:
        P = np.arange(w, w + pad)
        assert np.array_equal(np.triu(img[np.ix_(P, P)]), np.eye(pad))
        assert not np.any(img[np.ix_(P, np.arange(w + pad, h + pad))])
        assert not np.any(img[:w, w:w + pad])


def test_front_factor_non_positive_pivot_in_the_pivot_block(hip_ctx):
    w, c = 300, 500
    A = _front_matrix(w + c, 3)
    A[150, 150] = -1.0
    _front_factor(hip_ctx, A, w, expect=api.SPP_NOT_POSDEF)


def test_front_factor_indefinite_contribution_block_is_not_a_failure(hip_ctx):
    """S is the parent's business: a non-positive diagonal entry that only shows up in S is not a failed pivot"""
    w, c = 300, 500
    A = _front_matrix(w + c, 4)
    R11, R12, _ = _front_reference(A, w)
    A[w + 5, w + 5] = R12[:, 5] @ R12[:, 5] - 1.0          # S[5, 5] = -1
    out, _, _ = _front_factor(hip_ctx, A, w)
    R11, R12, S = _front_reference(A, w)
    assert S[5, 5] < 0
    iu = np.triu_indices(c)
    assert np.abs(out[w:, w:][iu] - S[iu]).max() / np.abs(A).max() < 1e-13
    assert np.abs(out[:w, w:] - R12).max() / np.abs(R12).max() < 1e-11


# ---- substitution accuracy on ill-conditioned systems ---------------------------------------------------------------
def _refined(A, b, lu, iters=3):
    """the solution refined with residuals in extended precision (as tests/parity.py does for the sparse systems)"""
    Al = A.astype(np.longdouble)
    bl = b.astype(np.longdouble)
    x = sla.lu_solve(lu, b).astype(np.longdouble)
    for _ in range(iters):
        r = bl - Al @ x
        x = x + sla.lu_solve(lu, r.astype(np.float64)).astype(np.longdouble)
    return x, Al


@pytest.mark.parametrize("n", [100, 257, 640, 1000, 3000])
def test_posv_accuracy_on_ill_conditioned_systems(hip_ctx, n):
    """forward and normwise backward error of spp_dense_posv within 4x LAPACK's own (np.linalg.solve): partial last
    blocks (100, 257, 1000, 3000) and chains of many hops (3000: 24 block rows)"""
    rng = np.random.default_rng(n)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    b = rng.standard_normal(n)
    for cond in (1e2, 1e6, 1e10, 1e12):
        A = (Q * np.logspace(0, -np.log10(cond), n)) @ Q.T
        A = 0.5 * (A + A.T)
        dA = api.DeviceArray.from_host(hip_ctx, np.asfortranarray(A).ravel(order="F"))
        db = api.DeviceArray.from_host(hip_ctx, b)
        assert hip_ctx._check(hip_ctx.lib.spp_dense_posv(hip_ctx.h, dA.ptr, n, n, db.ptr)) == 0
        x = db.download()
        dA.free(); db.free()
        xl = np.linalg.solve(A, b)
        xr, Al = _refined(A, b, sla.lu_factor(A))
        nx = float(np.linalg.norm(xr))

        def fwd(v):
            return float(np.linalg.norm(v.astype(np.longdouble) - xr)) / nx

        def bwd(v):   # ||A v - b|| / (||A|| ||v|| + ||b||), ||A||_2 = 1 by construction
            r = Al @ v.astype(np.longdouble) - b.astype(np.longdouble)
            return float(np.linalg.norm(r)) / (float(np.linalg.norm(v)) + float(np.linalg.norm(b)))

        # (an error floor of one ulp: LAPACK's own error can come out as ~0 by luck at cond 1e2)
        assert fwd(x) <= 4 * max(fwd(xl), EPS), (cond, fwd(x), fwd(xl))
        assert bwd(x) <= 4 * max(bwd(xl), EPS), (cond, bwd(x), bwd(xl))


# ---- state across calls -------------------------------------------------------------------------------------------
def _lowrank_spd(n, seed, r=64):
    rng = np.random.default_rng(seed)
    V = rng.standard_normal((n, r))
    A = V @ V.T / r
    A[np.diag_indices(n)] += 1.0 + rng.random(n)
    return A, rng.standard_normal(n)


def _check_factor(A, R, seed=0):
    """R^T R = A: in full up to 1000, by four random probe vectors above (|(R^T R - A) v| <= bound * |A|_max |v|_1)"""
    n = A.shape[0]
    if n <= 1000:
        return np.abs(R.T @ R - A).max() / np.abs(A).max()
    V = np.random.default_rng(seed).standard_normal((n, 4))
    E = R.T @ (R @ V) - A @ V
    return (np.abs(E).max(axis=0) / np.abs(V).sum(axis=0)).max() / np.abs(A).max()


def test_one_allocation_through_a_sequence_of_sizes(hip_ctx):
    """factor + solve sizes up and down through ONE device allocation on one context: the streamed launch's epochs and
    order table, the fused chain's monotonic counters, the block inverses' half form and the substitution's check
    constants carry over between calls -- every recurrence of a size must give the same bits, every result be right"""
    seq = [3000, 700, 5633, 3000, 4224, 129, 3000]
    nmax = max(seq)
    dA = api.DeviceArray(hip_ctx, nmax * nmax)
    db = api.DeviceArray(hip_ctx, nmax)
    seen = {}
    try:
        for n in seq:
            A, b = _lowrank_spd(n, n)
            buf = np.zeros(nmax * nmax); buf[:n * n] = A.ravel()     # symmetric: row-major == column-major
            dA.upload(buf)
            bb = np.zeros(nmax); bb[:n] = b
            db.upload(bb)
            assert hip_ctx._check(hip_ctx.lib.spp_dense_posv(hip_ctx.h, dA.ptr, n, n, db.ptr)) == 0
            R = np.triu(dA.download()[:n * n].reshape((n, n), order="F"))
            x = db.download()[:n]
            assert _check_factor(A, R) < 1e-13, n
            assert np.abs(A @ x - b).max() / np.abs(b).max() < 1e-12, n
            if n in seen:
                assert np.array_equal(R, seen[n][0]) and np.array_equal(x, seen[n][1]), "size %d: other bits than before" % n
            else:
                seen[n] = (R, x)
    finally:
        dA.free(); db.free()


def test_per_step_factor_reports_an_early_non_positive_pivot(hip_ctx):
    """6000 rows = 47 tile rows: the first two steps run the per-step schedule before the streamed launch takes over; a
    pivot of step 1 fails there. NOT_POSDEF, and the next factorization on the context is right."""
    n = 6000
    A, _ = _lowrank_spd(n, 21)
    B = A.copy()
    B[200, 200] = -1.0
    dA = api.DeviceArray.from_host(hip_ctx, B.reshape(-1))
    st = hip_ctx.lib.spp_dense_potrf_upper(hip_ctx.h, dA.ptr, n, n)
    assert st == api.SPP_NOT_POSDEF, (st, hip_ctx.last_error())
    dA.upload(A.reshape(-1))
    assert hip_ctx._check(hip_ctx.lib.spp_dense_potrf_upper(hip_ctx.h, dA.ptr, n, n)) == 0
    R = np.triu(dA.download().reshape((n, n), order="F"))
    dA.free()
    assert _check_factor(A, R) < 1e-13
