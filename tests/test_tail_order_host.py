"""Host-only: the workgroup order of the streamed dense factor (spp_tail_order_host). With a tile
mask the trailing tile rows whose every tile lags (i - first(i, j) > D) are numbered in front of all others, provided
they take at most half of the resident workgroups and leave room for the live demand of the rest; otherwise, and always
without a mask or with the switch off, the table is the sorted one (row by row). Everything is restated here in plain
Python from the rule, not from the library's code. No GPU needed."""
import numpy as np
import pytest

from slam_plus_plus_amd import api, synth

NB = 128
RESIDENT = [0, 1, 16, 64, 104, 128, 256, 304, 512, 4096]


def _patterns(nblk, rng):
    idx = np.arange(nblk)
    yield "diagonal", idx, idx
    I, J = np.triu_indices(nblk)
    yield "full", I, J
    keep = J - I <= max(2, nblk // 12)
    yield "band", I[keep], J[keep]
    keep = (J - I <= max(2, nblk // 12)) | (J >= nblk - max(3, nblk // 9))
    yield "band+border", I[keep], J[keep]
    keep = (J - I <= max(2, nblk // 40)) | (J >= nblk - max(3, nblk // 4))
    yield "thin band+wide border", I[keep], J[keep]
    keep = (I == J) | (J >= nblk - 5)
    yield "arrow", I[keep], J[keep]
    for d in (0.002, 0.02):
        keep = rng.random(I.size) < d
        yield "random%g" % d, I[keep], J[keep]


def _rows(words, Tc):
    """listed tiles per tile row: the diagonal always, nothing below it (as the launch forms its step words)"""
    return [[j for j in range(i, Tc) if j == i or (int(w) >> j) & 1] for i, w in enumerate(words)]


def _first(rows, i, j):
    for k in range(i):
        if i in rows[k] and j in rows[k]:
            return k
    return i


def _sorted_table(rows, beta=0.0):
    tiles = [(i, j) for i, r in enumerate(rows) for j in r]
    return sorted(tiles, key=lambda t: t[0] + beta * t[1])   # (stable: ties keep row-by-row order)


def _check(tag, n, words, has_rhs, resident, beta=0.0):
    Tr, Tc = len(words), (n // NB + 1 if has_rhs else len(words))
    rows = _rows(words, Tc)
    base = _sorted_table(rows, beta)
    tiles, info = api.tail_order_host(n, words, has_rhs, resident, True, beta)
    what = (tag, n, has_rhs, resident, info)
    # it is the plan of the launch that takes the whole factorization (spp_tail_plan_host, tests/test_tail_plan_host.py), and
    # the rows above are that plan's step words
    plan = api.tail_plan_host(n, words, has_rhs=has_rhs, tail_rows=64, resident=resident, early=1, beta=beta)
    assert plan["tiles"] == tiles and plan["info"] == info, what
    assert plan["rowbits"] == [(1 << Tc) - 1] + [sum(1 << j for j in r) for r in rows], what
    # a permutation of the listed tiles
    assert len(tiles) == len(base) and sorted(tiles) == sorted(base), what
    widest = max(len(r) for r in rows)
    D = resident // widest
    assert info["widest"] == widest and info["rows_resident"] == D, what
    ne, rs = info["n_early"], info["r_star"]
    # E in front, and with E removed the table is today's
    E, rest = tiles[:ne], tiles[ne:]
    assert rest == [t for t in base if t not in set(E)], what
    assert E == [t for t in base if t[0] >= rs], what          # whole trailing rows, in the base order among themselves
    first = {t: _first(rows, *t) for t in base}
    lag = {t: t[0] - first[t] > D for t in base}
    # the longest trailing run of rows in which every tile lags
    r_ref = Tr
    while r_ref > 0 and all(lag[(r_ref - 1, j)] for j in rows[r_ref - 1]):
        r_ref -= 1
    cand = [t for t in base if t[0] >= r_ref]
    others = [t for t in base if t[0] < r_ref]
    demand = max([sum(1 for t in others if first[t] <= r <= t[0]) for r in range(Tr)] + [0])
    use = resident > 0 and 0 < len(cand) <= resident // 2 and resident - len(cand) >= demand
    if use:
        assert ne == len(cand) and rs == r_ref and info["live_demand"] == demand, what + (r_ref, len(cand), demand)
        assert all(lag[t] for t in E), what
        assert ne <= resident // 2 and resident - ne >= demand, what
        # no tile outside E has a producer inside E: producers of (i, j) are the tiles (k, i), (k, j) of the steps it applies
        for (i, j) in rest:
            for k in range(i):
                if i in rows[k] and j in rows[k]:
                    assert k < rs, what
    else:
        assert ne == 0 and rs == Tr and tiles == base, what + (r_ref, len(cand), demand)
    # switch off, or no mask: the old table exactly
    off, info_off = api.tail_order_host(n, words, has_rhs, resident, False, beta)
    assert off == base and info_off["n_early"] == 0, what
    return ne


@pytest.mark.parametrize("bs,nblk", [(6, 43), (6, 150), (6, 400), (6, 871), (3, 1237), (6, 1365)])
@pytest.mark.parametrize("has_rhs", [True, False])
def test_table_obeys_the_rule_for_every_pattern_and_resident_count(bs, nblk, has_rhs):
    n = bs * nblk
    rng = np.random.default_rng(nblk)
    used = 0
    for tag, i1, i2 in _patterns(nblk, rng):
        words, _ = api.tile_mask_host(n, bs, i1, i2, has_rhs, True)
        for resident in RESIDENT:
            used += _check(tag, n, words, has_rhs, resident) > 0
        _check(tag, n, words, has_rhs, 256, beta=0.5)
    if nblk >= 871:
        assert used > 0, "no pattern of this size ever seated tiles early: the cases do not exercise the rule"


def test_without_a_mask_the_table_is_row_by_row():
    for n, has_rhs in [(5226, True), (5226, False), (1280, True), (128, True), (100, False)]:
        Tr, Tc = -(-n // NB), (n // NB + 1 if has_rhs else -(-n // NB))
        base = [(i, j) for i in range(Tr) for j in range(i, Tc)]
        for early in (True, False):
            tiles, info = api.tail_order_host(n, None, has_rhs, 256, early)
            assert tiles == base and info["n_early"] == 0 and info["r_star"] == Tr


def test_full_mask_seats_nothing_early_on_a_device_that_holds_few_rows():
    # every tile listed: a tile's first step is 0, so all rows behind D lag -- but they are far more than half the device
    n = 5226
    words, _ = api.tile_mask_host(n, 6, *np.triu_indices(871), True, True)
    tiles, info = api.tail_order_host(n, words, True, 256, True)
    assert info["n_early"] == 0 and tiles == [(i, j) for i in range(41) for j in range(i, 41)]


def _lam_of(prob):
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


def test_venice_mask_with_256_resident_seats_rows_31_to_40():
    """the flagship: 41 x 41 tiles (the right-hand side, column 5226, lies inside tile column 40), 651 listed. The widest
    row has 21 tiles, D = 256 // 21 = 12; the border columns 31 .. 40 are nonzero in every row, so the tiles of rows 31 .. 40
    apply step 0 and lag; tile (30, 30) does not (its column enters the band 10 rows earlier). Rows 31 .. 40 are the full
    triangle on the border columns: 55 tiles, the right-hand side's among them."""
    prob = synth.ba_problem(871, 530304, 2838740, 871, heavy_tail=True, name="venice871")
    words = api.schur_tile_mask_host(_lam_of(prob))
    assert len(words) == 41 and sum(bin(int(w)).count("1") for w in words) == 651
    ne = _check("venice871", 5226, words, True, 256)
    tiles, info = api.tail_order_host(5226, words, True, 256, True)
    assert info["r_star"] == 31 and info["rows_resident"] == 12
    assert tiles[:ne] == [(i, j) for i in range(31, 41) for j in range(i, 41)]
    assert ne == 55 and info["live_demand"] <= 256 - ne
    print("venice871:", info)
    # the same mask on half a device: refused, the old table
    tiles, info = api.tail_order_host(5226, words, True, 128, True)
    assert info["n_early"] == 0 and tiles == sorted(tiles)
