"""Host-only: the order in which a tile of the streamed dense factor applies its steps (tail_step_order in
spp_tile_plan.cpp), through spp_tail_step_order_host (mask -> order) and spp_schur_step_order_host (the
order a Schur plan carries), against a numpy restatement: steps sorted by the depth of their diagonal tile in the tile DAG
of the filled mask -- depth(k) = 1 + max depth(j) over j < k with tile (j, k) listed, the definition of the cost model in
tests/test_cam_order_host.py --, ties by k.

The plan carries the order under a dissected camera order only. A chain keeps k ascending by the rule itself (band,
bordered band, arrow); a block-diagonal mask does NOT -- its blocks are chains side by side, the rule interleaves them --
and keeps its ascending steps because its plan keeps the natural camera order: asserted on the plan. No GPU needed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import schur_fixtures as fx
from slam_plus_plus_amd import api, synth
from test_cam_order_host import _band_pairs, _graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB = 128


# ---- masks as boolean matrices Tr x Tc (upper tiles; the right-hand side column n lies in tile column n // 128) ---------
def _mask(kind, tr, n):
    tc = n // NB + 1
    I, J = np.triu_indices(tr)
    M = np.zeros((tr, tc), bool)
    w = max(1, tr // 8)
    if kind == "band":
        keep = J - I <= w
    elif kind == "band+border":
        keep = (J - I <= w) | (J >= tr - max(2, tr // 6))
    elif kind == "arrow":
        keep = (I == J) | (J >= tr - 2)
    elif kind == "blockdiag":
        keep = I // 3 == J // 3
    elif kind == "dissected":      # arc A, arc B (bands that do not see each other), separators coupled to both
        ta, tb = tr // 4, tr // 4 + tr // 3
        part = lambda t: np.where(t < ta, 0, np.where(t < tb, 1, 2))
        keep = ((part(I) == part(J)) & (J - I <= w)) | (part(J) == 2)
    elif kind == "three arcs":     # three chains of different lengths side by side, one separator row
        cut = np.array([0, tr // 5, tr // 5 + tr // 3, tr - 1, tr])
        part = lambda t: np.searchsorted(cut, t, side="right") - 1
        keep = ((part(I) == part(J)) & (J - I <= 1)) | (J == tr - 1)
    elif kind == "random":
        keep = (I == J) | (np.random.default_rng(tr).random(I.size) < 0.12)
    else:
        raise ValueError(kind)
    M[I[keep], J[keep]] = True
    return M


def _words(M):
    return np.array([sum(1 << int(j) for j in np.flatnonzero(r)) for r in M], np.uint64)


def _closed(M, n):
    """the filled mask as tile_mask_close forms it: diagonal tiles, the right-hand side's tile column, symbolic elimination"""
    M = M.copy()
    tr = M.shape[0]
    M[np.arange(tr), np.arange(tr)] = True
    M[:, n // NB] = True
    M &= np.triu(np.ones(M.shape, bool))
    for k in range(tr):
        r = np.flatnonzero(M[k, k + 1:]) + k + 1
        for a in r[r < tr]:
            M[a, r[r >= a]] = True
    return M


def _depth(F):
    tr = F.shape[0]
    depth = np.ones(tr, np.int64)
    for k in range(tr):
        above = np.flatnonzero(F[:k, k])
        if above.size:
            depth[k] = 1 + depth[above].max()
    return depth


KINDS = ["band", "band+border", "arrow", "blockdiag", "dissected", "three arcs", "random"]
# (n = 128 tr: the right-hand side has a tile column of its own; n = 128 tr - 6: it shares the last tile row's column, so
# every tile row reaches the last one)
SHAPES = [(tr, NB * tr - cut) for tr in (7, 12, 21, 41) for cut in (0, 6)]


@pytest.mark.parametrize("tr,n", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_depth_order_of_a_mask(kind, tr, n):
    M = _mask(kind, tr, n)
    F = _closed(M, n)
    so = api.tail_step_order_host(n, _words(M))
    assert np.array_equal(np.sort(so), np.arange(tr)), "not a permutation of the tile rows"
    assert np.array_equal(so, api.tail_step_order_host(n, _words(F))), "the filled mask gives another order than the raw one"
    depth = _depth(F)
    # the rule: by depth, ties by k
    assert np.array_equal(so, np.lexsort((np.arange(tr), depth)))
    # along any dependency path the depth grows, and the list follows it
    pos = np.empty(tr, np.int64)
    pos[so] = np.arange(tr)
    for j, k in zip(*np.nonzero(np.triu(F[:, :tr], 1))):
        assert depth[j] < depth[k] and pos[j] < pos[k], (j, k)
    # every tile: the list filtered by its step bits (both row tiles (k, i) and (k, j) listed, k below the tile's own row, as
    # the kernel filters) holds exactly the steps the bits select, once each -- and the bits select no step k > i
    for i, j in zip(*np.nonzero(F)):
        taken = [int(k) for k in so if k < i and F[k, i] and F[k, j]]
        want = np.flatnonzero(F[:, i] & F[:, j])
        assert want.max() == i, "a step beyond the tile's own row"
        assert sorted(taken) == want[want < i].tolist() and len(set(taken)) == len(taken), (i, j)
    if kind in ("band", "band+border", "arrow"):
        assert np.array_equal(so, np.arange(tr)), "%s: a chain keeps its steps ascending" % kind
    if kind == "blockdiag":   # (the rule alone interleaves the blocks: it is the plan that keeps such a matrix ascending, below)
        assert not np.array_equal(so, np.arange(tr))
    if kind == "dissected":
        ta, tb = tr // 4, tr // 4 + tr // 3
        m = min(ta, tb - ta)
        head = np.stack([np.arange(m), ta + np.arange(m)], 1).ravel()
        assert np.array_equal(so[:2 * m], head), "the arcs' steps are not interleaved by depth"
        assert np.array_equal(so[tb:], np.arange(tb, tr)), "the separators are not last, ascending"
        assert np.array_equal(np.sort(so[2 * m:tb]), np.arange(ta + m, tb) if tb - ta > ta else np.arange(m, ta))


def test_bad_arguments_are_rejected():
    lib = api.load_library()
    w = _words(_mask("band", 7, 896))
    out = np.zeros(64, np.int32)
    for n, nwords in ((896, 6), (0, 7), (64 * NB, 7)):
        assert lib.spp_tail_step_order_host(n, w.ctypes.data, nwords, out.ctypes.data) < 0
    assert lib.spp_tail_step_order_host(896, None, 7, out.ctypes.data) < 0
    assert lib.spp_tail_step_order_host(896, w.ctypes.data, 7, None) < 0


# ---- the order a Schur plan carries -------------------------------------------------------------------------------------
def _lam_of(prob):
    from oracle import spp_oracle as orc
    return orc.lambda_structure(prob)[0]


def _identity(so):
    return np.array_equal(so, np.arange(so.size))


@pytest.mark.parametrize("name", ["edges63", "edges32", "ba_small", "mis66"])
def test_small_fixtures_carry_the_identity(name):
    lam = fx.make(name)[0] if name in fx.ALL else _lam_of(synth.make(name))
    so = api.schur_step_order_host(lam, mis=name.startswith("mis"))
    assert _identity(so)


@pytest.mark.parametrize("dp", [6, 3])
def test_natural_camera_orders_carry_the_identity(dp):
    """chain, arrow and two components (a block-diagonal S: the RULE would interleave its blocks) keep the natural camera
    order, and with it the ascending steps"""
    nc = int(12 * NB / dp) - 2
    reach = int(NB / dp)
    h = nc // 2
    border = np.arange(nc - nc // 9, nc)
    graphs = {"chain": _band_pairs(nc, reach, False),
              "arrow": np.stack(np.meshgrid(np.arange(nc), border), -1).reshape(-1, 2),
              "two components": np.concatenate([_band_pairs(h, reach, False), _band_pairs(nc - h, reach, False) + h])}
    for tag, pairs in graphs.items():
        st, _ = _graph(nc, dp, pairs)
        assert not api.schur_cam_order_host(st)[1], tag
        so = api.schur_step_order_host(st)
        assert so.size == 12 and _identity(so), tag
    # sparse S: no tile mask, nothing to order
    assert api.schur_step_order_host(_graph(nc, dp, graphs["chain"])[0], sparse_S=True).size == 0


def test_a_ring_carries_the_depth_order_of_its_mask_on_every_shard():
    nc, dp = int(24 * NB / 6) - 2, 6
    st, adj = _graph(nc, dp, _band_pairs(nc, nc // 10, True))
    order, used, _, _ = api.schur_cam_order_host(st)
    assert used
    so = api.schur_step_order_host(st)
    assert so.size == 24 and not _identity(so)
    for rank, world in ((0, 2), (1, 2), (2, 3)):
        assert np.array_equal(api.schur_step_order_host(st, shard_rank=rank, shard_world=world), so)
    # it is the depth order of the mask of THAT camera order (restated from the co-visibility)
    pos = np.empty(nc, np.int64)
    pos[order] = np.arange(nc)
    t0, t1 = pos * dp // NB, (pos * dp + dp - 1) // NB
    M = np.zeros((24, 24), bool)
    I, J = np.nonzero(adj)
    for a in (t0, t1):
        for b in (t0, t1):
            M[a[I], b[J]] = True
    M &= np.triu(np.ones(M.shape, bool))
    assert np.array_equal(so, api.tail_step_order_host(nc * dp, _words(M)))


def test_venice_plan_interleaves_the_arcs_and_takes_the_separators_last():
    prob = synth.ba_problem(871, 530304, 2838740, 871, heavy_tail=True, name="venice871")
    lam = _lam_of(prob)
    order, used, _, chosen = api.schur_cam_order_host(lam)
    assert used and chosen["path"] == 32
    # arc A and arc B keep the natural order and A's cameras come first in it, so only the separators open with a drop
    tb = (int(np.flatnonzero(np.diff(order) < 0)[-1]) + 1) * 6 // NB
    ta = 9   # arcs of 9 and 12 tile rows, 20 separator rows
    assert tb == 21
    so = api.schur_step_order_host(lam)
    assert so.size == 41
    want = np.concatenate([np.stack([np.arange(ta), ta + np.arange(ta)], 1).ravel(), np.arange(2 * ta, 41)])
    assert np.array_equal(so, want), so
    assert np.array_equal(api.schur_step_order_host(lam, shard_rank=1, shard_world=2), so)


CHILD = r"""
import sys, json
sys.path.insert(0, %r)
from slam_plus_plus_amd import api, synth
from oracle import spp_oracle as orc
lam = orc.lambda_structure(synth.ba_problem(300, 4000, 16000, 5, heavy_tail=False, spread=0.06))[0]
print(json.dumps({"used": bool(api.schur_cam_order_host(lam)[1]),
                  "so": [api.schur_step_order_host(lam, shard_rank=r, shard_world=w).tolist() for r, w in ((0, 1), (0, 2), (1, 2))],
                  "checksum": api.schur_plan_host(lam)["checksum_all"]}))
"""


def _child(env):
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.strip().split("\n")[-1])


def test_switches_and_shards_see_one_order():
    """the 300-camera loop of tests/test_gpu_cam_order.py: the depth order by default, the same one with SPP_TAIL_MASK=0 (that
    switch changes scheduling, never bits) and on every shard; ascending with SPP_TAIL_STEP_ORDER=0 and with the natural
    camera order. The plan's uploaded lists do not change with SPP_TAIL_STEP_ORDER."""
    on, nomask = _child({}), _child({"SPP_TAIL_MASK": "0"})
    off, natural = _child({"SPP_TAIL_STEP_ORDER": "0"}), _child({"SPP_SCHUR_CAM_ORDER": "0"})
    ident = list(range(15))
    assert on["used"] and on["so"][0] != ident and sorted(on["so"][0]) == ident
    assert on["so"][0] == on["so"][1] == on["so"][2]
    assert nomask == on
    assert off["used"] and off["so"] == [ident] * 3 and off["checksum"] == on["checksum"]
    assert not natural["used"] and natural["so"] == [ident] * 3


# ---- the leading rows of a trailing run that is too large to be seated whole (tail_order_table's lead: early = 3) ------------
def _dissected_words(ta, tb, ts):
    tr = ta + tb + ts
    I, J = np.triu_indices(tr)
    part = lambda t: np.where(t < ta, 0, np.where(t < ta + tb, 1, 2))
    M = np.zeros((tr, tr + 1), bool)
    keep = (part(I) == part(J)) | (part(J) == 2)
    M[I[keep], J[keep]] = True
    n = NB * tr
    return n, _words(_closed(M, n)), _closed(M, n)


@pytest.mark.parametrize("ta,tb,ts", [(9, 12, 20), (4, 5, 16), (2, 3, 2), (6, 6, 12)])
@pytest.mark.parametrize("resident", [0, 1, 32, 64, 150, 256, 304, 1000])
def test_leading_rows_table(ta, tb, ts, resident):
    n, words, F = _dissected_words(ta, tb, ts)
    tr = ta + tb + ts
    listed = sorted((int(i), int(j)) for i, j in zip(*np.nonzero(F)))
    base, _ = api.tail_order_host(n, words, resident=resident, early=0)
    old, old_info = api.tail_order_host(n, words, resident=resident, early=1)
    new, info = api.tail_order_host(n, words, resident=resident, early=3)
    assert sorted(new) == listed and sorted(old) == listed, "not a permutation of the listed tiles"
    # the option off: the table as before (early = 1), which is the base order whenever it seats nothing
    if old_info["n_early"] == 0:
        assert old == base
    ne, r1 = info["n_early"], info["r_star"]
    if old_info["n_early"]:
        assert new == old and info == old_info, "the whole run fits: the leading rows change nothing"
        return
    if ne == 0:
        assert new == base and r1 == tr   # (nothing seated: the table is the base order, entry for entry)
        return
    # both conditions hold for what is seated, and fail for one row more
    demand = info["live_demand"]
    assert ne <= resident // 2 and resident - ne >= demand, (ne, resident, demand)
    E = new[:ne]
    rows_e = sorted(set(i for i, _ in E))
    r2 = rows_e[-1]
    assert rows_e == list(range(r1, r2 + 1)) and E == [t for t in base if r1 <= t[0] <= r2], "E is not whole leading rows in base order"
    if r2 + 1 < tr:
        more = ne + sum(1 for t in base if t[0] == r2 + 1)
        assert more > resident // 2 or resident - more < demand, "a further row would have met both conditions"
    # the numbering: E, rows < r1 by the depth of their row (ties: base order), rows > r2 in base order
    depth = _depth(F)
    front = [t for t in base if t[0] < r1]
    front.sort(key=lambda t: depth[t[0]])   # (stable)
    assert new[ne:] == front + [t for t in base if t[0] > r2]
    # progress: outside E every producer has a smaller index; a tile of E waits for rows < r1 or for earlier tiles of E
    index = {t: q for q, t in enumerate(new)}
    for (i, j), q in index.items():
        for k in range(i):
            if F[k, i] and F[k, j]:
                for prod in ((k, i), (k, j)):
                    if r1 <= i <= r2:
                        assert prod[0] < r1 or index[prod] < q
                    else:
                        assert index[prod] < q and not (i < r1 and r1 <= prod[0]), ((i, j), prod)


def test_leading_rows_of_the_venice_shape():
    """the mask of the Venice plan: 20 separator rows, 210 tiles against a bound of 128 -- as before nothing of them is seated
    (tests/test_gpu_dense_tail_order.py pins that refusal on the device); with the option rows 21 - 23, 57 tiles, and the
    arcs' rows interleaved behind them"""
    import scipy.sparse as sp
    from test_cam_order_host import _model
    prob = synth.ba_problem(871, 530304, 2838740, 871, heavy_tail=True, name="venice871")
    order = api.schur_cam_order_host(_lam_of(prob))[0]
    B = sp.csr_matrix((np.ones(prob.v0.size, np.float32), (prob.v1 - 871, prob.v0)), shape=(prob.npts, 871))
    adj = np.asarray(((B.T @ B) > 0).todense()) | np.eye(871, dtype=bool)
    fig, F = _model(adj, order, 6)
    assert (fig["tiles"], fig["path"]) == (662, 32)
    words = _words(F)
    old, old_info = api.tail_order_host(5226, words, resident=256, early=1)
    new, info = api.tail_order_host(5226, words, resident=256, early=3)
    assert old_info["n_early"] == 0 and old_info["r_star"] == 41 and old == api.tail_order_host(5226, words, resident=256, early=0)[0]
    assert info["r_star"] == 21 and info["n_early"] == 57 and sorted(set(t[0] for t in new[:57])) == [21, 22, 23], info
    rows = [t[0] for t in new[57:]]
    assert [r for q, r in enumerate(rows) if q == 0 or rows[q - 1] != r][:6] == [0, 9, 1, 10, 2, 11], "the arcs' rows are not interleaved"
    assert sorted(new) == sorted(old)
