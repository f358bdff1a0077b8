"""CPU: the reference machinery of tests/test_gpu_schur_sigma.py (tests/schur_sigma_ref.py), checked without a GPU.

  - exact_product is the longdouble product: against numpy's longdouble matmul on the reduced system of chain73.
  - the formula reference agrees with the refined longdouble inverse of the whole dense Lambda on tiny_shards, chain73
    and ba_interleaved (landmark-row-first observation blocks), every stored double, within 64 cond eps (measured:
    2.3e-16, 7.7e-16 and, at cond 1e5, 2.4e-13: S is rounded to float64 before it is inverted).
  - it agrees with solve_again_ref.covariance_ref (refined unit columns of Lambda itself) on a selection per fixture --
    the first, last (blind) and tile-straddling camera, the degree-1, 256-track, 257-track and unobserved landmark where
    the fixture has them, each with the cross blocks of its column -- within 64 cond eps, the bound of
    tests/test_solve_again_ref_host.py.
  - cond(Lambda) < solve_again_ref.COND_MAX on every fixture used; ba_interleaved is new to that bound."""
import numpy as np
import pytest

import schur_sigma_ref as ssg
import solve_again_ref as sar
import sparse_sigma_ref as sgr

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)


def _cond(name):
    if name != "ba_interleaved":
        return sar.condition(name)
    return float(np.linalg.cond(ssg.problem(name)[0].to_scipy().toarray()))


def test_exact_product_is_the_longdouble_product():
    lam = ssg.problem("chain73")[0]
    S = ssg.reduced_system(lam, ssg.parts("chain73"))[:300, :300].copy()
    rng = np.random.default_rng(3)
    X = np.linalg.inv(S).astype(LD) * (1 + LD(2) ** -60 * rng.integers(-8, 8, S.shape).astype(LD))
    ref = S.astype(LD) @ X
    err = float(np.abs(ssg.exact_product(S, X) - ref).max() / np.abs(ref).max())
    print("exact_product against longdouble matmul: %.3e" % err)
    assert err < 1e-18     # (the longdouble sum of 300 terms itself rounds at 300 * 2^-64 = 1.6e-17 of the largest term)


@pytest.mark.parametrize("name", ["tiny_shards", "chain73", "ba_interleaved"])
def test_the_formulas_agree_with_the_full_longdouble_inverse(name):
    lam = ssg.problem(name)[0]
    ref = ssg.reference(name)
    full = ssg.full_inverse_on_pattern(name)
    assert ref.shape == (lam.nvals,) and not np.any(np.isnan(ref)) and not np.any(np.isnan(full))
    err = sgr.column_errors(lam, ref, full)
    # S is formed in float64: its rounding, eps relative, reaches Sigma times cond -- the bound of the test below
    bound = 64 * _cond(name) * EPS
    print("%s: n = %d, largest block-column difference %.3e, bound %.3e" % (name, lam.n, err.max(), bound))
    assert np.all(err <= bound)
    if name == "ba_interleaved":
        P = ssg.parts(name)
        assert P.tr.any() and not P.tr.all(), "ba_interleaved stores observation blocks in both senses"


@pytest.mark.parametrize("name", ssg.FIXTURES)
def test_the_formulas_agree_with_refined_unit_columns_on_the_selection(name):
    lam = ssg.problem(name)[0]
    sel = ssg.selection(name)
    if name == "ba_interleaved":      # (not a fixture of solve_again_ref: its refinement on this Lambda)
        E, rows = sar.unit_columns(lam, sel)
        rf = sar._Refiner(lam)
        X = np.stack([rf.solve(np.ascontiguousarray(E[:, j])) for j in range(E.shape[1])], axis=1)
    else:
        _, X, rows = sar.covariance_ref(name, sel)
    pos, r, c, _ = sgr.pattern_index(lam)
    at = np.full(lam.n, -1, dtype=np.int64)
    at[rows] = np.arange(rows.size)
    m = at[c] >= 0
    cols = np.full(lam.nvals, np.nan)
    cols[pos[m]] = X[r[m], at[c[m]]]
    err = sgr.column_errors(lam, ssg.reference(name), cols)[sel]
    bound = 64 * _cond(name) * EPS
    print("%s: %d vertices, largest block-column difference %.3e, bound %.3e" % (name, len(sel), err.max(), bound))
    assert np.all(err <= bound)
    if name == "edges63_long":
        deg = np.bincount(ssg.parts(name).ob_lm, minlength=ssg.parts(name).lms.size)
        assert {0, 1, 256, 257} <= set(deg.tolist()) and len(sel) == 7


@pytest.mark.parametrize("name", ssg.FIXTURES)
def test_every_fixture_is_well_conditioned(name):
    cond = _cond(name)
    print("%s: cond(Lambda) = %.3e" % (name, cond))
    assert cond < sar.COND_MAX
