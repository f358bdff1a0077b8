"""Host-only: the camera order of the dense Schur plan (spp_schur_cam_order_host) and the tile-DAG cost
model behind it, against a numpy restatement. The model: filled 128 x 128 tile mask of S for a camera order, its listed
tiles, rank-128 updates and CRITICAL PATH (longest chain of diagonal tiles, depth(k) = 1 + max depth(j) over j < k with
tile (j, k) listed), cost = max(path 36.5 us, updates 2.0 us / 256) + 45 us. The rule cuts closed camera loops only and
only for a modelled gain of a tenth; everything else keeps the natural order, entry for entry. No GPU needed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import schur_fixtures as fx
from slam_plus_plus_amd import api, synth
from slam_plus_plus_amd.blockcsc import structure_from_pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB = 128
T_STEP, T_UPDATE, T_START, RESIDENT = 36.5, 2.0, 45.0, 256


# ---- graphs: cameras 0 .. nc-1 (width dp), one two-observer landmark per co-visible pair -----------------------------------
def _graph(nc, dp, pairs):
    dl = 3 if dp == 6 else 2
    pairs = np.unique(np.sort(np.asarray(pairs, np.int64).reshape(-1, 2), axis=1), axis=0)
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    nl = pairs.shape[0]
    dim = np.array([dp] * nc + [dl] * nl, np.int32)
    lm = nc + np.arange(nl)
    rows = np.concatenate([pairs[:, 0], pairs[:, 1]])
    cols = np.concatenate([lm, lm])
    st = structure_from_pairs(dim, rows, cols)[0]
    adj = np.eye(nc, dtype=bool)
    adj[pairs[:, 0], pairs[:, 1]] = adj[pairs[:, 1], pairs[:, 0]] = True
    return st, adj


def _band_pairs(nc, reach, ring):
    i = np.repeat(np.arange(nc), reach)
    j = i + np.tile(np.arange(1, reach + 1), nc)
    if ring:
        return np.stack([i, j % nc], axis=1)
    keep = j < nc
    return np.stack([i[keep], j[keep]], axis=1)


def _cams_per_tiles(dp):
    return NB // np.gcd(NB, dp)   # cameras between two tile boundaries that are camera boundaries too


def _cases():
    for dp in (6, 3):
        per_tile = NB / dp
        for tr in (8, 24, 40, 64):
            nc = int(tr * per_tile) - 2
            if nc * dp // NB + 1 > 64:
                nc = (63 * NB) // dp
            reach = max(2, int(per_tile * max(1, tr // 16)))
            yield "chain-%d-%d" % (dp, tr), nc, dp, _band_pairs(nc, reach, False), None
            # (band = reach on both sides: the two separators take a fifth of the ring, whole-tile arcs fit at every size
            # here and hide 3 of 8 ... 24 of 64 steps of the chain: accepted, all of them)
            yield "ring-fifth-%d-%d" % (dp, tr), nc, dp, _band_pairs(nc, nc // 10, True), True
            if tr <= 24:   # (every camera sees nearly every other: millions of pairs beyond that, nothing new)
                yield "ring-wide-%d-%d" % (dp, tr), nc, dp, _band_pairs(nc, int(nc * 0.49), True), False
            border = np.arange(nc - max(3, nc // 9), nc)
            yield "arrow-%d-%d" % (dp, tr), nc, dp, np.stack(np.meshgrid(np.arange(nc), border), -1).reshape(-1, 2), False
            h = nc // 2
            two = np.concatenate([_band_pairs(h, reach, False), _band_pairs(nc - h, reach, False) + h])
            yield "two-components-%d-%d" % (dp, tr), nc, dp, two, False
        nc = int(8 * per_tile)
        yield "dense-%d" % dp, nc, dp, np.stack(np.triu_indices(nc), 1), False


CASES = list(_cases())


# ---- the model in numpy -----------------------------------------------------------------------------------------------
def _model(adj, order, dp):
    nc = adj.shape[0]
    n = nc * dp
    Tr, Tc = -(-n // NB), n // NB + 1
    pos = np.empty(nc, np.int64)
    pos[np.asarray(order)] = np.arange(nc)
    t0, t1 = pos * dp // NB, (pos * dp + dp - 1) // NB
    M = np.zeros((max(Tr, Tc) + 1, Tc + 1), bool)
    I, J = np.nonzero(adj)
    for a in (t0, t1):
        for b in (t0, t1):
            M[a[I], b[J]] = True
    M = M[:Tr, :Tc]
    M[np.arange(Tr), np.arange(Tr)] = True
    M[:, n // NB] = True
    M &= np.triu(np.ones((Tr, Tc), bool))
    upd = 0
    for k in range(Tr):
        r = np.flatnonzero(M[k, k + 1:]) + k + 1
        for a in r[r < Tr]:
            M[a, r[r >= a]] = True
            upd += int((r >= a).sum())
    depth = np.ones(Tr, np.int64)
    for k in range(Tr):
        above = np.flatnonzero(M[:k, k])
        if above.size:
            depth[k] = 1 + depth[above].max()
    path = int(depth.max())
    return dict(tiles=int(M.sum()), updates=upd, path=path, cost_us=max(path * T_STEP, upd * T_UPDATE / RESIDENT) + T_START), M


def tr_of(tag):
    return int(tag.rsplit("-", 1)[1])


def _same(a, b):
    return all(a[k] == b[k] for k in ("tiles", "updates", "path")) and abs(a["cost_us"] - b["cost_us"]) < 1e-9


def _check_accepted(adj, order, dp, natural, chosen):
    nc = adj.shape[0]
    assert np.array_equal(np.sort(order), np.arange(nc)), "not a permutation"
    al = _cams_per_tiles(dp)
    # arc A, arc B, separators: both arcs whole tiles (B and the separators start on a tile boundary), natural order inside
    asc = lambda x: bool(np.all(np.diff(x) > 0))
    splits = [(a, b) for a in range(al, nc, al) for b in range(al, nc - a, al)
              if asc(order[:a]) and asc(order[a:a + b]) and asc(order[a + b:]) and not adj[np.ix_(order[:a], order[a:a + b])].any()]
    assert splits, "no tile-aligned split into two arcs that do not see each other, in natural order each"
    a, b = max(splits, key=lambda s: min(s))
    A, B = order[:a], order[a:a + b]
    assert not adj[np.ix_(A, B)].any(), "a block couples the two arcs"
    ref, M = _model(adj, order, dp)
    ta, tb = A.size * dp // NB, (A.size + B.size) * dp // NB
    assert not M[:ta, ta:tb].any(), "a listed tile couples the two arcs"
    assert _same(ref, chosen), (ref, chosen)
    assert chosen["cost_us"] <= 0.9 * natural["cost_us"]
    assert chosen["path"] < natural["path"]


@pytest.mark.parametrize("tag,nc,dp,pairs,accept", CASES, ids=[c[0] for c in CASES])
def test_model_and_rule_match_the_numpy_restatement(tag, nc, dp, pairs, accept):
    st, adj = _graph(nc, dp, pairs)
    order, used, natural, chosen = api.schur_cam_order_host(st)
    ref, _ = _model(adj, np.arange(nc), dp)
    assert _same(ref, natural), (ref, natural)
    if accept is not None:
        assert used == accept, (tag, natural, chosen)
    if tag.startswith("chain"):
        assert not used, "an open chain keeps the natural order"
    if used:
        _check_accepted(adj, order, dp, natural, chosen)
    else:
        assert np.array_equal(order, np.arange(nc)) and _same(natural, chosen)
    # the model of a GIVEN order (a rotation and a reversal): nothing is chosen
    for given in (np.roll(np.arange(nc), nc // 3), np.arange(nc)[::-1]):
        o2, used2, nat2, got = api.schur_cam_order_host(st, order=given)
        assert not used2 and np.array_equal(o2, given) and _same(nat2, natural)
        assert _same(_model(adj, given, dp)[0], got), (tag, got)
    # every landmark shard's plan holds the same order
    if used or tr_of(tag) <= 24:
        for rank, world in ((0, 2), (1, 2)):
            o3, used3, _, ch3 = api.schur_cam_order_host(st, shard_rank=rank, shard_world=world)
            assert used3 == used and np.array_equal(o3, order) and _same(ch3, chosen), (tag, rank, world)
    # sparse S keeps the natural order, and so does the MIS cut (a graph of one width: the same cameras tied by
    # camera-camera blocks; whichever of them the cut keeps as poses stay in their natural order)
    o4, used4, _, _ = api.schur_cam_order_host(st, sparse_S=True)
    assert not used4 and np.array_equal(o4, np.arange(nc))
    if tag.startswith("ring-fifth") and tr_of(tag) <= 24:
        p = np.unique(np.sort(np.asarray(pairs, np.int64).reshape(-1, 2), axis=1), axis=0)
        one = structure_from_pairs(np.full(nc, dp, np.int32), p[:, 0], p[:, 1])[0]
        o5, used5, _, _ = api.schur_cam_order_host(one, mis=True)
        assert not used5 and np.array_equal(o5, np.arange(o5.size)) and 0 < o5.size < nc


def _lam_of(prob):
    from oracle import spp_oracle as orc
    return orc.lambda_structure(prob)[0]


def test_venice_shape_is_accepted_with_a_shorter_chain():
    prob = synth.ba_problem(871, 530304, 2838740, 871, heavy_tail=True, name="venice871")
    lam = _lam_of(prob)
    order, used, natural, chosen = api.schur_cam_order_host(lam)
    assert (natural["tiles"], natural["updates"], natural["path"]) == (651, 5740, 41)   # (the mask of tests/test_tile_mask_host.py)
    assert used and chosen["path"] < 41, chosen
    print("venice871: natural %s, chosen %s" % (natural, chosen))
    # co-visibility from the graph, then the same checks as above
    import scipy.sparse as sp
    B = sp.csr_matrix((np.ones(prob.v0.size, np.float32), (prob.v1 - 871, prob.v0)), shape=(prob.npts, 871))
    adj = np.asarray(((B.T @ B) > 0).todense()) | np.eye(871, dtype=bool)
    _check_accepted(adj, order, 6, natural, chosen)
    assert (chosen["tiles"], chosen["updates"], chosen["path"]) == (662, 5971, 32)


@pytest.mark.parametrize("name", ["edges63", "edges32", "ba_small", "mis66"])
def test_small_fixtures_keep_the_natural_order(name):
    lam = fx.make(name)[0] if name in fx.ALL else _lam_of(synth.make(name))
    mis = name.startswith("mis")
    order, used, _, _ = api.schur_cam_order_host(lam, mis=mis)
    assert not used and np.array_equal(order, np.arange(order.size))


CHILD = r"""
import sys, json
sys.path.insert(0, %r)
import numpy as np
from slam_plus_plus_amd import api, synth
from oracle import spp_oracle as orc
lam = orc.lambda_structure(synth.ba_problem(300, 4000, 16000, 5, heavy_tail=False, spread=0.06))[0]
out = {"used": bool(api.schur_cam_order_host(lam)[1])}
for rank, world in ((0, 1), (0, 2), (1, 2)):
    d = api.schur_plan_host(lam, rank, world)
    out["%%d/%%d" %% (rank, world)] = [d["n_sblk"], d["checksum"]]
print(json.dumps(out))
"""


def _child(env):
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.strip().split("\n")[-1])


def test_switch_off_keeps_the_natural_order_and_shards_agree():
    """a 300-camera loop (the shape of tests/test_gpu_cam_order.py): accepted by default, the natural order with
    SPP_SCHUR_CAM_ORDER=0; SPP_TAIL_MASK=0 does not change the order (that switch promises the same bits with and without
    the mask); the block list of S -- the same blocks at other positions -- keeps its length"""
    on, off, nomask = _child({}), _child({"SPP_SCHUR_CAM_ORDER": "0"}), _child({"SPP_TAIL_MASK": "0"})
    assert on["used"] and not off["used"]
    assert nomask == on
    for key in ("0/1", "0/2", "1/2"):
        assert on[key][1] != off[key][1], "the plan did not change with the order"
    assert on["0/1"][0] == off["0/1"][0]
