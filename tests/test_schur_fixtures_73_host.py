"""Host-only: the 7 x 3 fixtures of the Schur stage (tests/schur_fixtures_73.py) against the edges they exist for, as
the host plan sees them -- the sibling of test_schur_ref.py::test_guided_fixture_reaches_its_edges. No GPU needed."""
import numpy as np
import pytest

import schur_fixtures as fx
import schur_fixtures_73 as fx73
import schur_ref
from slam_plus_plus_amd import api

PAIR_CHUNK = 2048   # spp_schur_plan.cpp: block products per work item of the S accumulation

_CACHE = {}


def _problem(name):
    if name not in _CACHE:
        _CACHE[name] = fx73.make(name)
    return _CACHE[name]


@pytest.mark.parametrize("name", sorted(fx73.ALL))
def test_landmark_blocks_are_well_conditioned(name):
    lam, eta = _problem(name)
    conds = fx.landmark_conds(lam, schur_ref.guided_elim(lam))
    print(name, "largest landmark condition %.3f" % conds.max())
    assert conds.max() <= fx.COND_MAX


@pytest.mark.parametrize("name", sorted(fx73.ALL))
def test_fixture_reaches_its_edges(name):
    lam, eta = _problem(name)
    assert set(np.unique(lam.dim).tolist()) == {3, 7}
    el = schur_ref.guided_elim(lam)
    R = schur_ref.schur_ref(lam, eta, el)
    nc = R.poses.size
    assert R.dp == 7 and R.n_red == 7 * nc
    ku = R.k[np.triu_indices(nc, 1)]
    for k in fx.EDGE_COUNTS:
        assert np.any(ku == k), (name, k)
    assert ku.max() >= 2 * PAIR_CHUNK + 1
    if name == "edges73":
        assert R.n_red == 2240 and R.n_red % 128 == 64, "17.5 tiles: the rhs column lies inside the last tile"
        straddle = [c for c in range(nc) if (7 * c) // 128 != (7 * c + 6) // 128]
        assert len(straddle) >= 10, "cameras that straddle a tile boundary"
        assert np.diff(R.lm_ptr).max() == 256
    else:
        assert R.n_red == 896 and R.n_red % 128 == 0, "the rhs column is the first padding column"
    blind = np.flatnonzero(R.obs_count == 0)
    assert any(R.has_A[:, c].sum() + R.has_A[c, :].sum() - 2 * R.has_A[c, c] > 0 for c in blind)
    assert (np.triu(R.has_A, 1) & (R.k_all == 0)).sum() >= 2, "A blocks of cameras without a shared landmark"
    track = np.diff(R.lm_ptr)
    for sparse in (False, True):
        d = api.schur_plan_host(lam, sparse_S=sparse)
        k = np.array([R.k_all[i1, i2] for i1, i2 in R.pattern])
        assert d["nc"] == nc and d["nl"] == R.lms.size and d["no"] == R.obs_pose.size
        assert d["n_pairs"] == int((track * (track + 1) // 2).sum())
        assert d["n_sblk"] == len(R.pattern)
        assert d["n_items"] == int(np.maximum(1, (k + PAIR_CHUNK - 1) // PAIR_CHUNK).sum())
        assert d["n_multi"] == int((k > PAIR_CHUNK).sum()) and d["n_multi"] > 0
