"""Host-only: the 128 x 128 tile mask of a dense reduced system and its symbolic fill (spp_tile_mask_host,
spp_schur_tile_mask_host: what the streamed dense factor uses to skip structurally zero tiles of S) against a plain numpy
elimination. Block sizes 7, 6 and 3 do not divide 128, so blocks straddle tile edges in both directions (7-wide blocks at
other places than 6-wide ones: only every 7th tile boundary is a block boundary). No GPU needed."""
import numpy as np
import pytest

from slam_plus_plus_amd import api, synth

NB = 128


def _ref_mask(n, bs, i1, i2, has_rhs, fill=True):
    """tiles touched by the corners of the blocks, diagonal tiles, the rhs tile column; then for k ascending every pair
    of nonzero tiles (k, a), (k, b), k < a <= b, fills (a, b). Returns (bool mask Tr x Tc, tile updates)."""
    Tr, Tc = -(-n // NB), (n // NB + 1 if has_rhs else -(-n // NB))
    M = np.zeros((Tr, Tc), bool)
    a, b = np.minimum(i1, i2).astype(np.int64), np.maximum(i1, i2).astype(np.int64)
    for r in (a * bs // NB, np.minimum(a * bs + bs - 1, n - 1) // NB):       # first / last row of the block
        for c in (b * bs // NB, np.minimum(b * bs + bs - 1, n - 1) // NB):   # first / last column
            M[r, c] = True   # (a corner below the diagonal, of a diagonal block, goes with the triangle below)
    M[np.arange(Tr), np.arange(Tr)] = True
    if has_rhs:
        M[:, n // NB] = True
    M &= np.triu(np.ones((Tr, Tc), bool))
    upd = 0
    for k in range(Tr):
        r = [j for j in range(k + 1, Tc) if M[k, j]]
        for a in r:
            if a < Tr:
                for b in r:
                    if b >= a:
                        if fill:
                            M[a, b] = True
                        upd += int(M[a, b])
    return M, upd


def _unpack(words, Tc):
    return np.array([[(int(w) >> j) & 1 for j in range(Tc)] for w in words], bool).reshape(len(words), Tc)


def _patterns(nblk, rng):
    idx = np.arange(nblk)
    yield "diagonal", idx, idx
    I, J = np.triu_indices(nblk)
    yield "full", I, J
    keep = J - I <= max(2, nblk // 12)
    yield "band", I[keep], J[keep]
    keep = (J - I <= max(2, nblk // 12)) | (J >= nblk - max(3, nblk // 9))
    yield "band+border", I[keep], J[keep]
    keep = (I == J) | (J >= nblk - 5)
    yield "arrow", I[keep], J[keep]
    keep = (I == J) | (I < 4)
    yield "arrow-up", I[keep], J[keep]   # a full first block row: everything fills
    for d in (0.002, 0.02):
        keep = rng.random(I.size) < d
        yield "random%g" % d, I[keep], J[keep]
    keep = rng.random(I.size) < 0.01
    yield "random-lower", J[keep], I[keep]   # blocks given in the lower triangle mark the upper tile


@pytest.mark.parametrize("bs,nblk", [(6, 43), (6, 64), (6, 150), (6, 871), (3, 300), (3, 1237), (2, 64), (6, 1365),
                                     (7, 92), (7, 128), (7, 330)])
@pytest.mark.parametrize("has_rhs", [True, False])
def test_mask_and_fill_match_a_numpy_elimination(bs, nblk, has_rhs):
    n = bs * nblk
    rng = np.random.default_rng(nblk)
    for tag, i1, i2 in _patterns(nblk, rng):
        for fill in (True, False):
            words, upd = api.tile_mask_host(n, bs, i1, i2, has_rhs, fill)
            M, upd_ref = _ref_mask(n, bs, i1, i2, has_rhs, fill)
            assert len(words) == M.shape[0], (tag, len(words))
            got = _unpack(words, M.shape[1])
            assert all(int(w) >> M.shape[1] == 0 for w in words), (tag, "bits beyond the last tile column")
            assert np.array_equal(got, M), (tag, fill, np.argwhere(got != M)[:5])
            assert upd == upd_ref, (tag, fill, upd, upd_ref)


def test_n_not_a_multiple_of_the_block_size_and_tile_edges():
    # n = 128 k exactly: the right-hand side column opens a tile column of its own
    for n, bs in [(256, 2), (384, 6), (130, 6), (127, 6), (129, 3), (644, 7), (896, 7), (130, 7)]:
        nblk = -(-n // bs)
        I, J = np.triu_indices(nblk)
        keep = (J - I) % 7 == 0
        words, upd = api.tile_mask_host(n, bs, I[keep], J[keep], True, True)
        M, upd_ref = _ref_mask(n, bs, I[keep], J[keep], True)
        assert np.array_equal(_unpack(words, M.shape[1]), M) and upd == upd_ref, (n, bs)


def test_more_than_64_tile_columns_means_no_mask():
    n = 64 * NB            # 64 tile rows + the right-hand side's tile column
    words, _ = api.tile_mask_host(n, 6, [0], [0], True, True)
    assert len(words) == 0
    words, _ = api.tile_mask_host(n - 1, 6, [0], [0], True, True)
    assert len(words) == 64


def _lam_of(prob):
    """block pattern of Lambda (upper triangle, BlockCSC-like) of a two-width problem, straight from its edge list"""
    nb = prob.dim.size
    lo, hi = np.minimum(prob.v0, prob.v1), np.maximum(prob.v0, prob.v1)
    key = np.unique(np.concatenate([hi * nb + lo, np.arange(nb) * (nb + 1)]))
    col, row = key // nb, key % nb
    col_ptr = np.zeros(nb + 1, np.int64)
    np.add.at(col_ptr, col + 1, 1)

    class Lam:
        pass
    lam = Lam()
    lam.nb, lam.dim, lam.col_ptr, lam.row_idx = nb, prob.dim.astype(np.int32), np.cumsum(col_ptr), row.astype(np.int64)
    return lam


def _schur_ref_mask(prob):
    """the tiles of S from the graph: every pair of observers of a landmark, by a sparse product"""
    import scipy.sparse as sp
    dims = prob.dim
    is_lm = dims == dims.min()
    pose_of = np.cumsum(~is_lm) - 1
    lm_of = np.cumsum(is_lm) - 1
    nc, dp = int((~is_lm).sum()), int(dims.max())
    v0, v1 = prob.v0, prob.v1
    cam = np.where(is_lm[v0], v1, v0)
    pt = np.where(is_lm[v0], v0, v1)
    assert (~is_lm[cam]).all() and is_lm[pt].all()
    B = sp.csr_matrix((np.ones(cam.size, np.float32), (lm_of[pt], pose_of[cam])), shape=(int(is_lm.sum()), nc))
    C = sp.triu((B.T @ B).tocsr()).tocoo()
    return _ref_mask(nc * dp, dp, C.row, C.col, True), nc * dp


@pytest.mark.parametrize("name", ["ba_small", "ba_banded", "ba_interleaved", "ba_medium"])
def test_schur_plan_mask_matches_the_graph(name):
    prob = synth.make(name)
    (M, _), n = _schur_ref_mask(prob)
    lam = _lam_of(prob)
    for rank, world in [(0, 1), (0, 2), (1, 2), (2, 3)]:
        # the mask of a sharded plan covers the landmarks of every shard: the exchanged S is the sum over the ranks
        words = api.schur_tile_mask_host(lam, rank, world)
        assert np.array_equal(_unpack(words, M.shape[1]), M), (name, rank, world)


def test_venice_shape_has_651_tiles_and_5740_updates():
    """the benchmark's flagship problem (871 cameras on a circle, 530 304 points, 2 838 740 observations, seed 871): S is a
    cyclic band -- after fill a band of 11 tiles per row plus a border of 10 tile columns; treated as dense it has 861
    tiles and 11 480 updates"""
    prob = synth.ba_problem(871, 530304, 2838740, 871, heavy_tail=True, name="venice871")
    lam = _lam_of(prob)
    words = api.schur_tile_mask_host(lam)
    (M, upd), n = _schur_ref_mask(prob)
    assert n == 5226 and len(words) == 41
    got = _unpack(words, 41)
    assert np.array_equal(got, M)
    assert int(got.sum()) == 651 and upd == 5740
    # and the same through the block list: the counts the block-list entry point reports
    _, upd_full = api.tile_mask_host(n, 6, *np.triu_indices(871), True, True)
    assert upd_full == 11480
    # the last 21 tile rows are a full triangle, the rows before them hold at most band + border
    assert all(got[i, i:].all() for i in range(20, 41))
    assert max(int(got[i].sum()) for i in range(20)) <= 21
