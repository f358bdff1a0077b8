"""The Levenberg-Marquardt scalars and robust weights of spp_geometry.hip -- edge_chi2, edge_hessian_maxdiag,
lm_gain_denominator, edge_robust_weights and the ||dx|| of the six update entry points -- against longdouble / exactly summed
references at n = 1, 255, 256, 257 and 65537 (one workgroup, a full one, a tail of one, and more than 256 partials, where the
second stage of the reduction makes a second pass), each called twice and required to return the same bits.

Error bounds (first order in eps = 2^-52), from the kernels' operation order:
* a sum over n items is a tree of depth 8 inside each 256-wide workgroup, then ONE workgroup whose thread t adds the partials
  t, t + 256, ... in order (ceil(nwg / 256) additions) and a second tree of depth 8: every term passes through at most
  16 + ceil(nwg / 256) additions;
* r^T Om r is evaluated as sum_i r_i (sum_j Om_ij r_j): at most 2 rd + 1 roundings on the way of any product, relative to
  |r|^T |Om| |r| (NOT to the term: a dense Om cancels inside it);
so |chi2 - exact| <= (2 rd + 17 + ceil(nwg / 256)) eps sum_e |r_e|^T |Om_e| |r_e|, and likewise with 3 (gain denominator: two
products and a sum per entry) or 1 (norms) in place of 2 rd + 1. (The figure this test was first given, (rd^2 + 10 + ceil(nwg /
256)) eps sum |terms|, counts rd^2 roundings where the chain of any one product has 2 rd + 1 and measures against the terms,
inside which a dense Om cancels; it is kept as a second assertion, since on these well-conditioned Om it is the smaller of the
two for rd 2 and 3 and the kernel meets it by a factor of 20.) A maximum is exact up to the rounding of the winning diagonal
entry: (2 rd + 1) eps max_c |J_c|^T |Om| |J_c|."""
import math

import numpy as np
import pytest

from slam_plus_plus_amd import api

pytestmark = pytest.mark.gpu
SIZES = [1, 255, 256, 257, 65537]
EPS = 2.0 ** -52
LD = np.longdouble


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def _up(ctx, a, dtype=np.float64):
    return api.DeviceArray.from_host(ctx, np.ascontiguousarray(a, dtype=dtype).ravel())


def _fsum_ld(t):
    """the exact sum of longdouble terms, rounded once: each term split into two doubles, math.fsum over all of them"""
    t = np.asarray(t, dtype=LD).ravel()
    hi = t.astype(np.float64)
    lo = (t - hi.astype(LD)).astype(np.float64)
    return math.fsum(hi.tolist() + lo.tolist())


def _passes(n_items):
    nwg = (n_items + 255) // 256
    return 16 + (nwg + 255) // 256


def _spd(rng, n, rd):
    """dense SPD information matrices (n, rd, rd), condition number of a few"""
    a = rng.normal(size=(n, rd, rd))
    return np.einsum("eij,ekj->eik", a, a) / rd + np.eye(rd)[None] * 0.5


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("rd", [2, 3, 6])
def test_chi2(ctx, rd, n):
    rng = np.random.default_rng(100 * rd + n % 97)
    r, Om = rng.normal(size=(n, rd)) * np.exp(rng.normal(size=(n, 1))), _spd(rng, n, rd)
    terms = np.einsum("ei,eij,ej->e", r.astype(LD), Om.astype(LD), r.astype(LD))
    absum = float(np.einsum("ei,eij,ej->e", np.abs(r).astype(LD), np.abs(Om).astype(LD), np.abs(r).astype(LD)).sum())
    ref = _fsum_ld(terms)
    dr, dO = _up(ctx, r), _up(ctx, Om.transpose(0, 2, 1))       # column-major blocks (symmetric anyway)
    got = ctx.edge_chi2_device(n, rd, dr.ptr, dO.ptr)
    again = ctx.edge_chi2_device(n, rd, dr.ptr, dO.ptr)
    bound = (2 * rd + 1 + _passes(n)) * EPS * absum
    first_guess = (rd * rd + 10 + (((n + 255) // 256) + 255) // 256) * EPS * float(np.abs(terms).sum())
    print("chi2 rd %d n %d: |got - exact| = %.3g, bound %.3g (first guess %.3g), exact %.17g" % (rd, n, abs(got - ref), bound, first_guess, ref))
    assert got == again
    assert abs(got - ref) <= bound
    assert abs(got - ref) <= first_guess      # no bound for a dense Om, smaller for rd 2 and 3, and met with room to spare
    dr.free(), dO.free()


def test_chi2_of_an_unsupported_width_is_an_error(ctx):
    d = _up(ctx, np.ones(64))
    with pytest.raises(api.SppError, match="-6"):
        ctx.edge_chi2_device(2, 4, d.ptr, d.ptr)
    d.free()


SHAPES = [(2, 6, 3), (3, 3, 3), (6, 6, 6), (3, 6, 3)]


def _hdiag(J, Om, rd, d):
    """(n, d) diagonals of J^T Om J in longdouble and their |.| counterparts; J (n, rd * d) column-major"""
    Jm = J.reshape(-1, d, rd).astype(LD)                         # [e, column, row]
    O = Om.astype(LD)
    return np.einsum("eci,eij,ecj->ec", Jm, O, Jm), np.einsum("eci,eij,ecj->ec", np.abs(Jm), np.abs(O), np.abs(Jm))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("shape", SHAPES)
def test_hessian_maxdiag(ctx, shape, n):
    """the maximum planted in J0 or in J1, in the first edge, the last edge of a full workgroup, the last edge (the lone edge
    of a tail workgroup at n = 257 and 65537)"""
    rd, d0, d1 = shape
    rng = np.random.default_rng(1000 * rd + 10 * d0 + n % 89)
    J0, J1, Om = rng.uniform(-1, 1, size=(n, rd * d0)), rng.uniform(-1, 1, size=(n, rd * d1)), _spd(rng, n, rd)
    dO, dJ = _up(ctx, Om.transpose(0, 2, 1)), [_up(ctx, J0), _up(ctx, J1)]
    base = [np.einsum("eci,eij,ecj->ec", J.reshape(n, d, rd), Om, J.reshape(n, d, rd), optimize=True) for J, d in ((J0, d0), (J1, d1))]
    top = max(float(b.max()) for b in base)
    seen = set()
    for e in sorted({0, min(255, n - 1), n - 1}):
        for side, (J, d) in enumerate(((J0, d0), (J1, d1))):
            Jp = J.copy()
            col = (e + side) % d
            Jp[e, rd * col:rd * (col + 1)] *= 8.0 * math.sqrt(top / float(base[side][e, col]))   # this entry becomes 64 top
            dJ[side].upload(Jp)
            h, ha = _hdiag(Jp[e:e + 1], Om[e:e + 1], rd, d)
            ref = float(h.max())
            assert h.argmax() == col and ref > 32 * top                      # the planted entry IS the maximum, by far
            got = ctx.edge_hessian_maxdiag_device(n, rd, d0, d1, dJ[0].ptr, dJ[1].ptr, dO.ptr)
            assert got == ctx.edge_hessian_maxdiag_device(n, rd, d0, d1, dJ[0].ptr, dJ[1].ptr, dO.ptr)
            assert abs(got - ref) <= (2 * rd + 1) * EPS * float(ha.max()), (e, side, got, ref)
            seen.add((e, side))
            dJ[side].upload(J)
    assert len(seen) == 2 * len({0, min(255, n - 1), n - 1})
    zero = [_up(ctx, np.zeros_like(J0)), _up(ctx, np.zeros_like(J1))]
    assert ctx.edge_hessian_maxdiag_device(n, rd, d0, d1, zero[0].ptr, zero[1].ptr, dO.ptr) == 0.0
    for a in dJ + zero + [dO]:
        a.free()


@pytest.mark.parametrize("shape", [(2, 3, 3), (3, 3, 2), (6, 6, 3), (3, 2, 2), (4, 6, 3)])
def test_hessian_maxdiag_of_an_unsupported_shape_is_an_error(ctx, shape):
    d = _up(ctx, np.ones(256))
    with pytest.raises(api.SppError, match="-6"):
        ctx.edge_hessian_maxdiag_device(2, *shape, d.ptr, d.ptr, d.ptr)
    d.free()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("alpha, sign", [(0.37, 1.0), (0.0, 1.0), (2.5, -1.0), (0.0, -1.0)])
def test_lm_gain_denominator(ctx, alpha, sign, n):
    """dx . (alpha dx + eta): a positive total, alpha = 0, and totals that are negative (eta against dx)"""
    rng = np.random.default_rng(n % 83 + int(10 * alpha))
    dx = rng.normal(size=n) * np.exp(rng.normal(size=n))
    eta = sign * np.abs(rng.normal(size=n)) * np.sign(dx) * (1 if sign > 0 else 8 * (1 + alpha)) + 0.1 * rng.normal(size=n)
    terms = dx.astype(LD) * (LD(alpha) * dx.astype(LD) + eta.astype(LD))
    absum = float((np.abs(dx) * (abs(alpha) * np.abs(dx) + np.abs(eta))).sum())
    ref = _fsum_ld(terms)
    assert (ref < 0) == (sign < 0)
    d1, d2 = _up(ctx, dx), _up(ctx, eta)
    got = ctx.lm_gain_denominator_device(n, d1.ptr, d2.ptr, alpha)
    assert got == ctx.lm_gain_denominator_device(n, d1.ptr, d2.ptr, alpha)
    bound = (3 + _passes(n)) * EPS * absum
    print("gain n %d alpha %g: |got - exact| = %.3g, bound %.3g, exact %.17g" % (n, alpha, abs(got - ref), bound, ref))
    assert abs(got - ref) <= bound
    d1.free(), d2.free()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("rd", [2, 3, 6])
def test_robust_weights(ctx, rd, n):
    """Huber weights: 1 up to x = param, param / x beyond, x = |r| / scale. Rows 0 .. 3 (as far as n allows): r = 0; x == param
    exactly (|r| = 3, scale 2, param 1.5: every operation exact, so w must be exactly 1); x one ulp above (|r| the next double
    after 3: r^2, its root and the division by 2 round the same way with or without a fused multiply-add, so the float64
    recomputation is exact, too); x = 1e150. Every other row against longdouble: the sum of rd squares, a root and two
    divisions are rd + 3 roundings."""
    scale, param = 2.0, 1.5
    rng = np.random.default_rng(rd + n % 79)
    r = rng.normal(size=(n, rd)) * np.exp(2 * rng.normal(size=(n, 1)))
    special = np.zeros((4, rd))
    special[1, rd - 1], special[2, 0], special[3, 1] = 3.0, np.nextafter(3.0, 4.0), 1e150
    k = min(4, n)
    r[:k] = special[:k]
    dr, dw = _up(ctx, r), api.DeviceArray(ctx, n)
    ctx.edge_robust_weights_device(n, rd, dr.ptr, dw.ptr, scale, param)
    w = dw.download()
    ctx.edge_robust_weights_device(n, rd, dr.ptr, dw.ptr, scale, param)
    assert np.array_equal(w, dw.download())
    x = np.sqrt((r.astype(LD) ** 2).sum(axis=1)) / LD(scale)
    ref = np.where(x <= param, LD(1), LD(param) / np.where(x > 0, x, 1))
    near = np.abs(x - param) <= 4 * EPS * param                 # within rounding of the kink both arms are within eps of 1
    err = np.abs(w.astype(LD) - ref) / ref
    assert (err[~near] <= (rd + 3) * EPS).all(), float(err[~near].max())
    assert (np.abs(w[near] - 1.0) <= 8 * EPS).all()
    assert w[0] == 1.0
    if n >= 4:
        x2 = math.sqrt(float(r[2, 0]) * float(r[2, 0])) / scale
        assert w[1] == 1.0 and x2 > param and w[2] == param / x2 and w[2] < 1.0
        assert w[3] == param / (1e150 / scale)
    assert (w > 0).all() and (w <= 1).all()
    assert n == 1 or ((x > param).any() and (x < param).any())
    dr.free(), dw.free()


@pytest.mark.parametrize("scale, param", [(0.0, 1.5), (-1.0, 1.5), (2.0, 0.0), (2.0, -0.5)])
def test_robust_weights_reject_a_non_positive_scale_or_parameter(ctx, scale, param):
    d = _up(ctx, np.ones(16))
    with pytest.raises(api.SppError, match="-1"):
        ctx.edge_robust_weights_device(4, 2, d.ptr, d.ptr, scale, param)
    d.free()


N_INTRINSICS = {1: 1, 255: 51, 256: 52, 257: 257, 65537: 13108}   # 5, 255, 260, 1285 and 65540 live entries


@pytest.mark.parametrize("n", SIZES)
def test_update_norms(ctx, n):
    """||dx|| from the six update entry points: se2_update and se3_update over n poses (3 n and 6 n entries), slam2d_update,
    slam3d_update and ba_update over n entries, ba_intrinsics_update over N_INTRINSICS[n] vertices. apply=False: the states
    are placeholders and must come back untouched. The entry points return the root of the device's sum: compared as squares,
    which adds the root's rounding and the squaring's (3 eps). se2_update reduces one value per pose (three squares: 3
    roundings), the others one square per entry.
    ba_intrinsics_update sums the 5 live entries of every vertex in ONE workgroup: below, at and past one pass of its 256
    threads, and many passes. Thread t adds its ceil(5 ni / 256) squares in order, then the tree of depth 8:
    |got^2 - exact| <= (1 + 8 + ceil(5 ni / 256) + 3) eps exact. The vertices sit at 6 i in a padded dx whose inert sixth
    entries hold 1e3: a kernel that counted them would miss the bound by orders of magnitude."""
    rng = np.random.default_rng(n % 71)
    dx = rng.normal(size=6 * n) * np.exp(rng.normal(size=6 * n))
    d, st, off = _up(ctx, dx), _up(ctx, np.ones(6 * n)), _up(ctx, np.zeros(1), np.int64)
    ni = N_INTRINSICS[n]
    live = rng.normal(size=(ni, 5)) * np.exp(rng.normal(size=(ni, 5)))
    padded = np.concatenate([live, np.full((ni, 1), 1e3)], axis=1)
    di, ioff = _up(ctx, padded), _up(ctx, 6 * np.arange(ni), np.int64)
    calls = {"se2": (lambda: ctx.se2_update_device(n, st.ptr, d.ptr, False), dx[:3 * n], 3 + _passes(n)),
             "se3": (lambda: ctx.se3_update_device(n, st.ptr, d.ptr, False), dx[:6 * n], 1 + _passes(6 * n)),
             "slam2d": (lambda: ctx.slam2d_update_device(n, st.ptr, d.ptr, 0, off.ptr, False), dx[:n], 1 + _passes(n)),
             "slam3d": (lambda: ctx.slam3d_update_device(n, st.ptr, d.ptr, 0, off.ptr, False), dx[:n], 1 + _passes(n)),
             "ba": (lambda: ctx.ba_update_device(0, st.ptr, off.ptr, 0, st.ptr, off.ptr, d.ptr, n, False), dx[:n], 1 + _passes(n)),
             "ba_intrinsics": (lambda: ctx.ba_intrinsics_update_device(ni, st.ptr, ioff.ptr, di.ptr, apply=False), live,
                               1 + 8 + (5 * ni + 255) // 256)}
    for name, (fn, entries, roundings) in calls.items():
        ref = _fsum_ld(entries.astype(LD) ** 2)
        got = fn()
        assert got == fn(), name
        bound = (roundings + 3) * EPS * ref
        print("%s n %d: |got^2 - exact| / exact = %.3g, bound %.3g" % (name, n, abs(got * got - ref) / ref, bound / ref))
        assert abs(got * got - ref) <= bound, name
    assert np.array_equal(st.download(), np.ones(6 * n))
    for b in (d, st, off, di, ioff):
        b.free()
