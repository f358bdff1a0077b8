"""Host-only: the 7 x 3 fixtures of the Schur stage (tests/schur_fixtures_73.py) against the edges they exist for, as
the host plan sees them -- the sibling of test_schur_ref.py::test_guided_fixture_reaches_its_edges -- and the shapes of
fx.ring (loop73, loop32, loop63, chain73) and tiny_shards against the conditions the GPU tests of the camera order, the clear by
tiles and the split API rely on: order accepted, tiles left unlisted, camera-camera blocks in both senses, the split pair
reversed, a shard without landmarks. No GPU needed."""
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
        _CACHE[name] = fx73.make_any(name)
    return _CACHE[name]


def _listed(words):
    return {(i, j) for i, w in enumerate(words) for j in range(64) if (int(w) >> j) & 1}


@pytest.mark.parametrize("name", sorted(fx73.ALL) + sorted(fx73.SHAPES) + sorted(fx.SHAPES))
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


# ---- the shapes of fx.ring: what the GPU tests of the camera order, the clear by tiles and the empty shard rely on -------
LOOPS = [("loop73", 7, 3, 330, 19, fx73.LOOP73_SPLIT), ("loop32", 3, 2, 300, 8, fx.LOOP32_SPLIT),
         ("loop63", 6, 3, 300, 15, fx.LOOP63_SPLIT)]


@pytest.mark.parametrize("name,dp,dl,nc,tile_rows,split", LOOPS, ids=[c[0] for c in LOOPS])
def test_loop_has_its_order_accepted_with_blocks_in_both_senses(name, dp, dl, nc, tile_rows, split):
    lam, eta = _problem(name)
    assert set(np.unique(lam.dim).tolist()) == {dl, dp} and int((lam.dim == dp).sum()) == nc
    assert -(-nc * dp // 128) == tile_rows
    conds = fx.landmark_conds(lam, schur_ref.guided_elim(lam))
    assert conds.max() <= fx.COND_MAX
    order, used, natural, chosen = api.schur_cam_order_host(lam)
    print(name, "largest landmark condition %.2f, natural %s, chosen %s" % (conds.max(), natural, chosen))
    assert used and chosen["path"] < natural["path"] == tile_rows, "the camera order of the loop is not accepted"
    al = 128 // np.gcd(128, dp)
    assert al == (64 if dp == 6 else 128), "the arc length of this width is 128 cameras (64 for 6-wide cameras)"
    assert np.array_equal(order[:al], np.arange(al)), "arc A is not the first whole arc length of cameras"
    words = api.schur_tile_mask_host(lam)
    assert len(words) == tile_rows
    assert len(_listed(words)) == natural["tiles"] < tile_rows * (tile_rows + 1) // 2, "every tile is listed"
    pos = np.empty(nc, np.int64)
    pos[order] = np.arange(nc)
    u, v = fx.ring_a_edges(nc)
    assert (pos[u] > pos[v]).any() and (pos[u] < pos[v]).any(), "camera-camera blocks in both senses"
    R = schur_ref.schur_ref(lam, eta, schur_ref.guided_elim(lam))
    assert R.has_A[split[0], split[1]] and R.k_all[split[0], split[1]] > PAIR_CHUNK, "the split pair has a camera-camera block"
    assert pos[split[0]] > pos[split[1]], "the split pair is not reversed"
    d = api.schur_plan_host(lam)
    assert d["n_multi"] >= 1, "no S block is split over several work items"
    assert d["nc"] == nc and d["n_items"] > d["n_sblk"]
    for rank in range(2):   # every landmark shard's plan holds the same order
        o2, used2, _, _ = api.schur_cam_order_host(lam, shard_rank=rank, shard_world=2)
        assert used2 and np.array_equal(o2, order)


def test_chain73_keeps_the_natural_order_and_has_unlisted_tiles():
    lam, eta = _problem("chain73")
    nc = int((lam.dim == 7).sum())
    assert nc == 92 and 7 * nc == 644
    assert all((128 * t) % 7 for t in range(1, 6)), "a camera straddles every tile boundary"
    order, used, natural, chosen = api.schur_cam_order_host(lam)
    assert not used and np.array_equal(order, np.arange(nc))
    words = api.schur_tile_mask_host(lam)
    assert len(words) == 6 and len(_listed(words)) == natural["tiles"] < 21
    # every camera that straddles a tile boundary has an off-diagonal block of S: blocks straddle in both directions
    R = schur_ref.schur_ref(lam, eta, schur_ref.guided_elim(lam))
    for t in range(1, 6):
        c = 128 * t // 7
        assert 7 * c < 128 * t < 7 * c + 7 and R.k_all[c, c] > 0 and R.k_all[c].sum() > R.k_all[c, c], t


@pytest.mark.parametrize("name", ["loop73", "chain73", "loop32", "edges73", "edges73_aligned"])
def test_plan_mask_is_the_numpy_mask_of_the_blocks_of_s(name):
    """the mask the Schur plan builds from the graph (every tile a block of S touches, both tiles of a camera that
    straddles a boundary in either direction, then the symbolic fill) against the numpy elimination of
    tests/test_tile_mask_host.py on the reference's block pattern of S"""
    from test_tile_mask_host import _ref_mask, _unpack
    lam, eta = _problem(name)
    R = schur_ref.schur_ref(lam, eta, schur_ref.guided_elim(lam))
    i1 = np.array([p[0] for p in R.pattern])
    i2 = np.array([p[1] for p in R.pattern])
    M, _ = _ref_mask(R.n_red, R.dp, i1, i2, True)
    for rank, world in [(0, 1), (0, 2), (1, 2)]:   # (a sharded plan's mask covers the landmarks of every shard)
        words = api.schur_tile_mask_host(lam, rank, world)
        assert np.array_equal(_unpack(words, M.shape[1]), M), (name, rank, world)
    straddling = [c for c in range(R.poses.size) if (R.dp * c) // 128 != (R.dp * c + R.dp - 1) // 128]
    assert straddling, "no camera straddles a tile boundary"


@pytest.mark.parametrize("name,dp", [("tiny_shards", 6), ("tiny_shards73", 7)])
def test_tiny_shards_leaves_a_shard_of_three_without_landmarks(name, dp):
    lam, eta = _problem(name)
    assert lam.dim.tolist() == [dp] * 4 + [3] * 2
    for sparse in (False, True):
        got = [api.schur_plan_host(lam, r, 3, sparse_S=sparse) for r in range(3)]
        assert [g["nl"] for g in got] == [1, 1, 0] and [g["no"] for g in got] == [2, 2, 0]
        assert all(g["nc"] == 4 for g in got)
    R = schur_ref.schur_ref(lam, eta, schur_ref.guided_elim(lam))
    assert np.triu(R.has_A, 1).sum() == 1
