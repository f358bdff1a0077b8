"""Host-only: everything the host decides for the streamed dense factor's launch (tail_plan in spp_tile_plan.cpp, DESIGN
section 28), through spp_tail_plan_host -- the function the launch itself calls: whether the region is one launch, its step
words (cut out of the caller's filled mask, also behind a per-step front), the step list as the kernel unpacks it, the
workgroup table. Everything is restated here in plain Python from the rule, not from the library's code. No GPU needed."""
import numpy as np
import pytest

from slam_plus_plus_amd import api
from test_tail_order_host import _patterns
from test_tail_step_order_host import _dissected_words

NB = 128
NO_STEP = api.TAIL_NO_STEP


def _starts(nblk):
    return sorted(set(f for f in (0, 1, nblk - 44, nblk - 2, nblk - 1) if 0 <= f < nblk))


def _ref_rowbits(filled, f, tr, tc):
    """the step words of the region behind the first f tile rows; filled: one int per tile row of the whole matrix, or None"""
    all_cols = (1 << tc) - 1
    out = [((filled[f - 1] >> f) & all_cols) if (f > 0 and filled is not None) else all_cols]
    for i in range(tr):
        w = (filled[f + i] >> f) if filled is not None else all_cols
        out.append(((w | 1 << i) & ~((1 << i) - 1)) & all_cols)
    return out


def _ref_table(rb, tr, tc, have_pre, resident, early):
    """the table without leading rows, the row panel in front of the region being step -1: the sorted
    (row by row) table, with the longest trailing run of tile rows whose every tile lags in front of it when that run takes
    at most half of the resident workgroups and leaves room for the live demand of the others"""
    rows = [set(j for j in range(i, tc) if (rb[i + 1] >> j) & 1) for i in range(tr)]
    base = [(i, j) for i in range(tr) for j in sorted(rows[i])]
    if not early or resident <= 0:
        return base, base, rows
    pre = set(j for j in range(tc) if (rb[0] >> j) & 1) if have_pre else set()

    def first(i, j):
        if i in pre and j in pre:
            return -1
        for k in range(i):
            if i in rows[k] and j in rows[k]:
                return k
        return i
    D = resident // max(len(r) for r in rows)
    fst = {t: first(*t) for t in base}
    r_ref = tr
    while r_ref > 0 and all(r_ref - 1 - fst[(r_ref - 1, j)] > D for j in rows[r_ref - 1]):
        r_ref -= 1
    cand = [t for t in base if t[0] >= r_ref]
    others = [t for t in base if t[0] < r_ref]
    live = np.zeros(tr + 1, np.int64)
    for t in others:
        live[max(fst[t], 0)] += 1
        live[t[0] + 1] -= 1
    demand = int(np.cumsum(live)[:tr].max()) if tr else 0
    if 0 < len(cand) <= resident // 2 and resident - len(cand) >= demand:
        return cand + others, base, rows
    return base, base, rows


def _assert_feeders_first(tiles, n_early, rows, what):
    """every tile comes behind the tiles (k, i), (k, j) that feed it -- but for the n_early tiles E seated in front, which come
    behind those of their feeders that are in E: nothing outside E is fed by E"""
    pos = {t: q for q, t in enumerate(tiles)}
    for (i, j), q in pos.items():
        for k in range(i):
            if i in rows[k] and j in rows[k]:
                for feeder in ((k, i), (k, j)):
                    assert pos[feeder] < q or (q < n_early and pos[feeder] >= n_early), what + ((i, j), feeder)
                    assert q < n_early or pos[feeder] >= n_early, what + ((i, j), feeder)


@pytest.mark.parametrize("cut", [0, 6])
@pytest.mark.parametrize("nblk", [3, 9, 46, 50])
def test_step_words_and_table_for_every_pattern_and_region_start(nblk, cut):
    """n = 128 nblk: the right-hand side has a tile column of its own; 6 less: it shares the last tile row's column"""
    n = NB * nblk - cut
    tc_all = n // NB + 1
    rng = np.random.default_rng(nblk)
    seated_behind_a_front = 0
    for tag, i1, i2 in _patterns(nblk, rng):
        words, _ = api.tile_mask_host(n, NB, i1, i2, True, True)
        filled = [int(w) for w in words]
        for f in _starts(nblk):
            tr, tc = nblk - f, tc_all - f
            what = (tag, n, f)
            plan = api.tail_plan_host(n, words, front=f, tail_rows=44, resident=256, early=1)
            if tr > 44:
                assert plan is None, what
                plan = api.tail_plan_host(n, words, front=f, tail_rows=64, resident=256, early=1)
            rb = _ref_rowbits(filled, f, tr, tc)
            assert plan["rowbits"] == rb, what
            want, base, rows = _ref_table(rb, tr, tc, f > 0, 256, True)
            assert sorted(plan["tiles"]) == base, what      # a permutation of the listed tiles of those words
            assert plan["tiles"] == want, what
            _assert_feeders_first(plan["tiles"], plan["info"]["n_early"], rows, what)
            seated_behind_a_front += f > 0 and want != base
            steps = ([-1] if f else []) + list(range(tr))
            assert plan["steps"] == steps + [NO_STEP] * (72 - len(steps)), what
            # the early switch off: the sorted table, the same words
            off = api.tail_plan_host(n, words, front=f, tail_rows=64, resident=256, early=0)
            assert off["tiles"] == base and off["rowbits"] == rb and off["info"]["n_early"] == 0, what
            # without a mask, or with the mask switched off: every tile right of the diagonal, the sorted table
            dense_rb = _ref_rowbits(None, f, tr, tc)
            dense = [(i, j) for i in range(tr) for j in range(i, tc)]
            for plan in (api.tail_plan_host(n, None, front=f, tail_rows=64), api.tail_plan_host(n, words, front=f, tail_rows=64, tail_mask=False)):
                assert plan["rowbits"] == dense_rb and plan["tiles"] == dense and plan["info"]["n_early"] == 0, what
    if nblk == 50:
        assert seated_behind_a_front, "no region behind a front ever seated tiles early: the cases do not exercise the row panel's word"


def test_resident_counts_behind_a_front():
    """the row panel in front of the region is step -1 of the rule: the border tiles of a bordered band lag from the start"""
    nblk, n = 50, NB * 50
    for tag, i1, i2 in _patterns(nblk, np.random.default_rng(nblk)):
        words, _ = api.tile_mask_host(n, NB, i1, i2, True, True)
        filled = [int(w) for w in words]
        for f in (6, 20):
            tr, tc = nblk - f, nblk + 1 - f
            rb = _ref_rowbits(filled, f, tr, tc)
            for resident in (0, 1, 64, 128, 304, 4096):
                plan = api.tail_plan_host(n, words, front=f, resident=resident, early=1)
                want, base, _ = _ref_table(rb, tr, tc, True, resident, True)
                assert plan["tiles"] == want and (plan["info"]["n_early"] > 0) == (want != base), (tag, f, resident)


def test_step_list():
    n, words, _ = _dissected_words(4, 5, 16)
    tr = 25
    so = api.tail_step_order_host(n, words)
    assert not np.array_equal(so, np.arange(tr))
    asc = list(range(tr))
    # the whole factorization: the passed order when it has one entry per tile row, with or without the mask in force
    for kw in ({}, {"tail_mask": False}, {"early": 0}):
        assert api.tail_plan_host(n, words, so, **kw)["steps"][:tr + 1] == so.tolist() + [NO_STEP]
    assert api.tail_plan_host(n, None, so)["steps"][:tr + 1] == so.tolist() + [NO_STEP]
    # another length: ascending
    for bad in (so[:-1], np.concatenate([so, [tr]]), None):
        assert api.tail_plan_host(n, words, bad)["steps"][:tr + 1] == asc + [NO_STEP]
    # behind a front: the row panel first, then ascending, whatever is passed
    for f in (1, 3, 24):
        for order in (so, so[:tr - f], np.arange(tr - f)[::-1], None):
            steps = api.tail_plan_host(n, words, order, front=f)["steps"]
            assert steps[:tr - f + 2] == [-1] + list(range(tr - f)) + [NO_STEP] and set(steps[tr - f + 2:]) <= {NO_STEP}
    # not a permutation: refused
    for bad in ([0] * tr, asc[:-1] + [tr], asc[:-1] + [-1], [1] + asc[1:], asc[:-1] + [127]):
        with pytest.raises(api.SppError) as e:
            api.tail_plan_host(n, words, bad)
        assert e.value.code == api.SPP_E_BADARG


@pytest.mark.parametrize("tr,f", [(1, 1), (7, 1), (8, 1), (9, 1), (63, 1), (64, 0)])
def test_step_list_packs_and_unpacks(tr, f):
    """tr + 1 entries behind a front (8: exactly one word and the terminator in the next, 63: the last entry of word 7), 64
    entries for the largest whole factorization: word 8 holds terminators only"""
    n = NB * (tr + f)
    perm = np.random.default_rng(tr).permutation(tr) if f == 0 else None
    plan = api.tail_plan_host(n, None, perm, front=f, has_rhs=False, tail_rows=64)
    want = ([-1] + list(range(tr))) if f else perm.tolist()
    assert len(plan["steps"]) == 72 and plan["steps"] == want + [NO_STEP] * (72 - len(want))
    assert len(plan["rowbits"]) == tr + 1 and len(plan["tiles"]) == tr * (tr + 1) // 2


def test_regions_the_launch_does_not_take_are_reported():
    n = NB * 10
    words, _ = api.tile_mask_host(n, NB, np.arange(10), np.arange(10), True, True)
    assert api.tail_plan_host(n, words) is not None
    assert api.tail_plan_host(n, words, front=10) is None and api.tail_plan_host(n, words, front=11) is None    # no tile row left
    assert api.tail_plan_host(n, words, tail_rows=9) is None and api.tail_plan_host(n, words, front=1, tail_rows=9) is not None
    assert api.tail_plan_host(n, words, tail_rows=0) is None and api.tail_plan_host(n, None, front=9, tail_rows=0) is None
    # 64 tile rows and the right-hand side in a 65th tile column
    assert api.tail_plan_host(NB * 64, None, tail_rows=64) is None and api.tail_plan_host(NB * 64 - 1, None, tail_rows=64) is not None
    assert api.tail_plan_host(NB * 64, None, front=1, tail_rows=64) is not None
    # (a bad step order is not looked at where the launch does not apply or does not use it)
    assert api.tail_plan_host(n, words, [0] * 10, tail_rows=9) is None and api.tail_plan_host(n, words, [0] * 9, front=1) is not None


@pytest.mark.parametrize("ta,tb,ts,resident,r_star", [(7, 8, 16, 256, 15), (4, 5, 16, 150, 9)])
def test_leading_rows_need_mask_switches_step_order_and_the_whole_factorization(ta, tb, ts, resident, r_star):
    """the separator rows lag and are too many to be seated whole (7, 8, 16: 152 tiles against a bound of 128): their leading
    rows go first only with a mask in force, SPP_TAIL_EARLY, a step order other than k ascending, no front and
    SPP_TAIL_EARLY_LEAD"""
    n, words, _ = _dissected_words(ta, tb, ts)
    tr = ta + tb + ts
    so = api.tail_step_order_host(n, words)
    kw0 = dict(resident=resident, early=3)
    lead = api.tail_plan_host(n, words, so, **kw0)
    plain = api.tail_plan_host(n, words, so, resident=resident, early=1)
    assert plain["info"]["n_early"] == 0 and plain["tiles"] == sorted(plain["tiles"])
    assert lead["info"]["n_early"] > 0 and lead["info"]["r_star"] == r_star and lead["tiles"] != plain["tiles"]
    assert sorted(lead["tiles"]) == plain["tiles"]
    assert (lead["tiles"], lead["info"]) == api.tail_order_host(n, words, resident=resident, early=3)
    for kw in (dict(step_order=np.arange(tr)), dict(step_order=None), dict(step_order=so[:-1]), dict(step_order=so, early=2),
               dict(step_order=so, tail_mask=False)):
        other = api.tail_plan_host(n, words, **dict(kw0, **kw))
        assert other["info"]["n_early"] == 0 and other["tiles"] == sorted(other["tiles"]), kw
    assert api.tail_plan_host(n, None, so, **kw0)["info"]["n_early"] == 0
    for f in (1, ta):
        assert api.tail_plan_host(n, words, so[:tr - f], front=f, **kw0) == api.tail_plan_host(n, words, None, front=f, resident=resident, early=1)
