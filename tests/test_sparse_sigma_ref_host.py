"""CPU: the reference machinery of tests/test_gpu_sparse_sigma.py (tests/sparse_sigma_ref.py), checked without a GPU.

  - the refined inverse of every connected component of at most 700 scalars of every designed fixture, and of the dense
    Lambda of the two damped pose graphs: max |I - Lambda X| <= 1e-16 with the product in longdouble (measured: <= 2e-18),
    and X symmetric to the same bound times its size;
  - no fixture is dropped: every system has a reference on every block column of its components up to 700 scalars and on
    the first, middle and last block of every clique of the larger ones (tree_hi, the two widest cliques of forest_c);
  - blocks_on_pattern round-trips Lambda itself bit for bit;
  - the refined inverse agrees with ssr.covariance_ref on ssr.marginal_selection(name) within 64 cond eps;
  - the conditions tests/test_sparse_solve_ref_host.py establishes: cond_2 = 80 on the designed fixtures (<= 100 asserted),
    below solve_again_ref.COND_MAX on the pose graphs."""
import numpy as np
import pytest

import solve_again_ref as sar
import sparse_fixtures as sf
import sparse_sigma_ref as sgr
import sparse_solve_ref as ssr

EPS = float(np.finfo(np.float64).eps)
RES_TOL = 1e-16
SYSTEMS = list(sf.NAMES) + list(ssr.POSE)


@pytest.mark.parametrize("name", SYSTEMS)
def test_refined_inverse_residual_and_symmetry(name):
    comps = sgr.components(name)
    inv = sgr.full_inverse(name)
    dense = [L for _, _, L in comps if L is not None]
    assert len(inv) == len(dense)
    assert all(s.size <= sgr.FULL_MAX or name in ssr.POSE for s, _ in inv)
    worst_r, worst_s = 0.0, 0.0
    for (s, X), L in zip(inv, dense):
        R = np.eye(s.size, dtype=np.longdouble) - L.astype(np.longdouble) @ X
        worst_r = max(worst_r, float(np.abs(R).max()))
        worst_s = max(worst_s, float(np.abs(X - X.T).max() / np.abs(X).max()))
    print("%s: %d components inverted, largest |I - Lambda X| %.3e, largest asymmetry %.3e" % (name, len(inv), worst_r, worst_s))
    assert worst_r <= RES_TOL and worst_s <= RES_TOL


def test_no_fixture_is_dropped():
    large = {}
    for name in SYSTEMS:
        lam = ssr.problem(name)[0]
        checked = set(int(v) for v in sgr.checked_vertices(name))
        for s, b, L in sgr.components(name):
            if L is not None:
                assert set(int(v) for v in b) <= checked, name
            else:
                large.setdefault(name, []).append(int(s.size))
        ref = sgr.reference_on_pattern(name)
        _, _, _, cb = sgr.pattern_index(lam)
        have = np.zeros(lam.nb, dtype=bool)
        have[cb[~np.isnan(ref[sgr.pattern_index(lam)[0]])]] = True
        assert set(int(v) for v in np.flatnonzero(have)) == checked, name
        assert len(checked) > 0, name
    assert large == {"tree_hi": [872], "forest_c": [1023, 1024]}, large
    fx = ssr.fixture("tree_hi")
    assert len(sgr.sampled_vertices("tree_hi")) >= 3 * len(fx.cliques) - 4      # (cliques of one or two blocks repeat one)
    assert len(sgr.sampled_vertices("forest_c")) == 6


@pytest.mark.parametrize("name", SYSTEMS)
def test_blocks_on_pattern_round_trips_lambda(name):
    lam = ssr.problem(name)[0]
    assert np.array_equal(sgr.blocks_on_pattern(lam, lam.to_dense(symmetric=False)), lam.vals[:lam.nvals])
    pos, r, c, cb = sgr.pattern_index(lam)
    assert np.array_equal(np.sort(pos), np.arange(lam.nvals)), "every double of vals belongs to one stored block"
    assert np.all(lam.base[cb] <= c) and np.all(c < lam.base[cb + 1])


@pytest.mark.parametrize("name", SYSTEMS)
def test_reference_agrees_with_covariance_ref(name):
    lam = ssr.problem(name)[0]
    sel = ssr.marginal_selection(name)
    cov = ssr.covariance_ref(name, sel)[0]
    ref = sgr.reference_on_pattern(name)
    bound = 64 * ssr.condition(name) * EPS
    checked = set(int(v) for v in sgr.checked_vertices(name))
    at, worst, n = 0, 0.0, 0
    for v in sel:
        d = int(lam.dim[v])
        if v in checked:
            p = int(lam.col_ptr[v + 1]) - 1
            blk = ref[lam.blk_off[p]:lam.blk_off[p] + d * d].reshape((d, d), order="F")
            worst = max(worst, float(np.abs(blk - cov[at:at + d, at:at + d]).max() / np.abs(blk).max()))
            n += 1
        at += d
    print("%s: %d diagonal blocks, largest difference %.3e (bound %.3e)" % (name, n, worst, bound))
    assert n >= 3 and worst <= bound


@pytest.mark.parametrize("name", SYSTEMS)
def test_conditions_hold(name):
    cond = ssr.condition(name)
    print("%s: cond %.3e" % (name, cond))
    assert cond < sar.COND_MAX if name in ssr.POSE else cond <= 100.0
