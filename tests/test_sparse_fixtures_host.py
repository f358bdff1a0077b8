"""The designed systems of tests/sparse_fixtures.py, checked on the host (no GPU): what makes the 1e-12 bound of
tests/test_gpu_sparse_fronts.py mean something.

  conditioning   every connected component has cond_2 <= 100: eps * cond ~ 2e-14, a margin of ~50 under the bound
  widths         the forest's clique widths are the designed ones, every block width 1..8 occurs in every fixture
  reference      the float64 solve refined with a longdouble residual has converged: another pass changes it by <= 1e-17
  sensitivity    scaling ONE stored block by 1 + 1e-9 moves the solution of its component by more than 1e-12 relative,
                 for every block of a sample of leaf, separator and coupling blocks: a front that loses or misplaces an
                 entry (a relative change of 1, not of 1e-9) is far outside the bound"""
import numpy as np
import pytest
import scipy.linalg as sla

import sparse_fixtures as sf

_cache = {}


def _fx(name):
    if name not in _cache:
        _cache[name] = sf.build(name)
    return _cache[name]


@pytest.mark.parametrize("name", sf.NAMES)
def test_components_are_well_conditioned(name):
    fx = _fx(name)
    worst = 0.0
    for L in fx.dense:
        ev = np.linalg.eigvalsh(L)
        assert ev[0] > 0
        worst = max(worst, ev[-1] / ev[0])
    print("%s: largest cond_2 over %d components %.1f" % (name, len(fx.dense), worst))
    assert worst <= 100.0


@pytest.mark.parametrize("name", sf.NAMES)
def test_block_widths_and_structure(name):
    fx = _fx(name)
    lam = fx.lam
    assert sorted(set(int(d) for d in lam.dim)) == list(range(1, 9)), "every block width 1..8 occurs"
    assert sum(s.size for s in fx.comp_scalars) == lam.n
    if name in sf.FOREST_WIDTHS:
        nc = len(sf.FOREST_WIDTHS[name])
        assert [g["width"] for g in fx.cliques[:nc]] == sf.FOREST_WIDTHS[name]
        assert [s.size for s in fx.comp_scalars[:nc]] == sf.FOREST_WIDTHS[name] and len(fx.comp_scalars) == nc + 1
        # complete block graphs: every pair of blocks of a component is stored (the last component is the forest's small tree)
        comp_of_block = np.zeros(lam.nb, dtype=np.int64)
        for c, blk in enumerate(fx.comp_blocks):
            comp_of_block[blk] = c
        stored = np.bincount(comp_of_block[lam.col_idx])
        assert [int(v) for v in stored[:nc]] == [b.size * (b.size + 1) // 2 for b in fx.comp_blocks[:nc]]
    else:
        # every leaf is coupled to a strict subset of its separator, with a gap in it somewhere in the fixture
        assert (fx.block_kind == 2).any() and (fx.block_kind == 0).any() and (fx.block_kind == 1).any()
    # the dense matrices and the block values agree
    A = lam.to_scipy()
    for s, L in zip(fx.comp_scalars, fx.dense):
        assert np.array_equal(A[s][:, s].toarray(), L)


def test_forest_widths_are_the_designed_ones():
    assert sorted(w for ws in sf.FOREST_WIDTHS.values() for w in ws) == [
        1, 15, 16, 17, 48, 49, 112, 113, 191, 192, 304, 305, 384, 385, 624, 625, 1023, 1024]


@pytest.mark.parametrize("name", sf.NAMES)
def test_reference_has_converged(name):
    fx = _fx(name)
    x2, _ = sf.reference(fx, passes=2)
    x3, change = sf.reference(fx, passes=3)
    print("%s: last refinement pass changes x by %.1e relative (largest over the components)" % (name, max(change)))
    assert max(change) <= 1e-17
    # its float64 image moves by a rounding tie at the most
    assert np.abs(x2 - x3).max() <= 2.0 ** -52 * np.abs(x3).max()


@pytest.mark.parametrize("name", sf.NAMES)
def test_every_sampled_block_moves_the_solution(name):
    fx = _fx(name)
    lam = fx.lam
    rng = np.random.default_rng(7)
    comp_of_scalar = np.zeros(lam.n, dtype=np.int64)
    local = np.zeros(lam.n, dtype=np.int64)
    for c, s in enumerate(fx.comp_scalars):
        comp_of_scalar[s] = c
        local[s] = np.arange(s.size)
    x_ref = sf.lapack_solution(fx)
    kinds = [k for k in range(3) if (fx.block_kind == k).any()]
    per_kind = -(-54 // len(kinds))
    smallest = {}
    n_sampled = 0
    sample = []
    for k in kinds:
        cand = np.flatnonzero(fx.block_kind == k)
        sample += [int(p) for p in rng.choice(cand, size=min(per_kind, cand.size), replace=False)]
    rest = np.setdiff1d(np.arange(lam.nnzb), sample)       # a kind with few blocks: the others make up for it
    sample += [int(p) for p in rng.choice(rest, size=min(max(0, 54 - len(sample)), rest.size), replace=False)]
    for p in sample:
        k = int(fx.block_kind[p])
        i, j = int(lam.row_idx[p]), int(lam.col_idx[p])
        c = comp_of_scalar[lam.base[i]]
        s = fx.comp_scalars[c]
        ri = local[lam.base[i]:lam.base[i + 1]]
        rj = local[lam.base[j]:lam.base[j + 1]]
        L = fx.dense[c].copy()
        L[np.ix_(ri, rj)] *= 1.0 + 1e-9
        if i != j:
            L[np.ix_(rj, ri)] *= 1.0 + 1e-9
        x = sla.cho_solve(sla.cho_factor(L), fx.eta[s])
        move = np.linalg.norm(x - x_ref[s]) / np.linalg.norm(x_ref[s])
        smallest[k] = min(smallest.get(k, np.inf), move)
        n_sampled += 1
    assert n_sampled >= 50, n_sampled
    print("%s: smallest relative move of x for a block scaled by 1 + 1e-9, over %d blocks: %s" % (
        name, n_sampled, ", ".join("%s %.2e" % (sf.KINDS[k], v) for k, v in smallest.items())))
    assert min(smallest.values()) > 1e-12
