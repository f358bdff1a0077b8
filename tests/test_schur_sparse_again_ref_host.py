"""CPU: the fixture and the reference tests/schur_sparse_again_ref.py adds (cliques63), checked without a GPU by the
criteria tests/test_schur_sigma_ref_host.py and tests/test_solve_again_ref_host.py apply to theirs.

  - cond(Lambda) < solve_again_ref.COND_MAX: the refined references are exact far below the 1e-10 floor of the criterion.
  - the fixture is what its description says: the tracks seen by all of A, all of G, G and 5 of A, M and 23 of A, L and 4 of
    G; degree-1 landmarks, one unobserved landmark; camera-camera blocks, one of them of two cameras without a shared
    landmark; n under 3000, so every block column is checked.
  - the formula reference (schur_sigma_ref.formulas on the refined inverse of S) agrees with the refined longdouble inverse
    of the whole dense Lambda on every stored double, and with refined unit columns of Lambda itself
    (solve_again_ref.covariance_ref) on the marginal vertices and the selection, within 64 cond eps.
  - E^T Lambda^-1 E from refined unit columns agrees with the longdouble inverse within that bound and is symmetric to it."""
import numpy as np

import schur_sigma_ref as ssg
import schur_sparse_again_ref as ssa
import solve_again_ref as sar
import sparse_sigma_ref as sgr

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
NAME = ssa.NEW


def test_the_fixture_is_well_conditioned_and_small_enough_for_every_block_column():
    lam = ssa.problem(NAME)[0]
    cond = sar.condition(NAME)
    print("%s: n = %d, cond(Lambda) = %.3e" % (NAME, lam.n, cond))
    assert cond < sar.COND_MAX
    assert lam.n < 3000 and lam.n <= ssg.N_ALL and ssg.checked_vertices(NAME).size == lam.nb


def test_the_fixture_is_the_designed_one():
    lam = ssa.problem(NAME)[0]
    P = ssg.parts(NAME)
    assert (P.dp, P.dl) == (6, 3) and P.cams.size == ssa.N_A + ssa.N_G + ssa.N_M + ssa.N_L + ssa.N_H + ssa.N_P
    assert np.array_equal(P.cams, np.arange(P.cams.size))
    deg = np.bincount(P.ob_lm, minlength=P.lms.size)
    count = dict(zip(*np.unique(deg, return_counts=True)))
    assert count[0] == 1 and count[1] == 2 * P.cams.size
    assert count[ssa.N_A] == 3 and count[ssa.N_G] == 3
    assert count[ssa.N_G + ssa.A_OF_G] == 1 and count[ssa.N_M + ssa.A_OF_M] == 1 and count[ssa.N_L + ssa.G_OF_L] == 1
    # the 360 reduced rows of A: one clique of the reduced system, and so is G
    for size, first in ((ssa.N_A, 0), (ssa.N_G, ssa.N_A)):
        l = int(np.flatnonzero(deg == size)[0])
        assert np.array_equal(np.sort(P.ob_cam[P.ob_lm == l]), np.arange(first, first + size))
    # camera-camera blocks off the diagonal, one of them between two cameras that share no landmark
    i, j = lam.row_idx[P.cc], lam.col_idx[P.cc]
    off = i != j
    assert off.sum() == 7
    shared = set()
    for l in np.flatnonzero(deg > 1):
        cs = P.ob_cam[P.ob_lm == l]
        shared |= {(int(a), int(b)) for a in cs for b in cs if a < b}
    lonely = [(int(a), int(b)) for a, b in zip(i[off], j[off]) if (int(a), int(b)) not in shared]
    assert len(lonely) == 1


def test_the_formulas_agree_with_the_full_longdouble_inverse_on_every_stored_double():
    lam = ssa.problem(NAME)[0]
    ref = ssa.reference(NAME)
    full = ssg.full_inverse_on_pattern(NAME)
    assert ref.shape == (lam.nvals,) and not np.any(np.isnan(ref)) and not np.any(np.isnan(full))
    err = sgr.column_errors(lam, ref, full)
    bound = 64 * sar.condition(NAME) * EPS
    print("%s: n = %d, largest block-column difference %.3e, bound %.3e" % (NAME, lam.n, err.max(), bound))
    assert np.all(err <= bound)


def test_the_formulas_and_the_covariance_agree_with_refined_unit_columns():
    lam = ssa.problem(NAME)[0]
    sel = sorted(set(ssg.selection(NAME)) | set(ssa.marginal_vertices(NAME).tolist()))
    cov, X, rows = sar.covariance_ref(NAME, sel)
    pos, r, c, _ = sgr.pattern_index(lam)
    at = np.full(lam.n, -1, dtype=np.int64)
    at[rows] = np.arange(rows.size)
    m = at[c] >= 0
    cols = np.full(lam.nvals, np.nan)
    cols[pos[m]] = X[r[m], at[c[m]]]
    err = sgr.column_errors(lam, ssa.reference(NAME), cols)[sel]
    bound = 64 * sar.condition(NAME) * EPS
    print("%s: %d vertices, largest block-column difference %.3e, bound %.3e" % (NAME, len(sel), err.max(), bound))
    assert np.all(err <= bound)
    exact = ssg.refined_inverse(lam.to_scipy().toarray())[:, rows]
    ecol = np.linalg.norm((X - exact).astype(np.float64), axis=0) / np.linalg.norm(exact.astype(np.float64), axis=0)
    err_cov = float(np.abs(cov - exact[rows].astype(np.float64)).max() / np.abs(exact[rows]).max())
    print("largest column error %.3e, covariance block error %.3e" % (ecol.max(), err_cov))
    assert np.all(ecol <= bound) and err_cov <= bound
    assert float(np.abs(cov - cov.T).max()) <= bound * float(np.abs(cov).max())
