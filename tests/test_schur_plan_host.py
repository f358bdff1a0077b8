"""Host-only: the symbolic Schur plan (spp_schur_plan_host -- guided ordering, observation lists, block pattern of S and
its per-block lists of block products; what CLinearSolver_Schur recomputes structurally in every call,
LinearSolver_Schur.cpp:771-838, LinearSolver_Schur.h:1699-1709, BlockMatrixFBS.inl:1147-1304). No GPU needed: the plan is
pure integer work on host threads; its result must not depend on their number, and it is pinned, list by list, by two
checksums recorded once (RECORDED below)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from slam_plus_plus_amd import api, synth
from oracle import spp_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import sys, json
sys.path.insert(0, %r)
from slam_plus_plus_amd import api, synth
from oracle import spp_oracle as orc
lam = orc.lambda_structure(synth.make(sys.argv[1]))[0]
d = api.schur_plan_host(lam, int(sys.argv[2]), int(sys.argv[3]), sys.argv[4] == "1")
d.pop("seconds")
print(json.dumps(d))
"""


def _plan(name, threads, rank=0, world=1, sparse=False, min_work=None):
    import json
    env = dict(os.environ, SPP_PLAN_THREADS=str(threads))
    if min_work is not None:
        env["SPP_PLAN_MIN_WORK"] = str(min_work)
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT, name, str(rank), str(world), "1" if sparse else "0"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.strip().split("\n")[-1])


@pytest.mark.parametrize("name", ["ba_small", "ba_interleaved", "ba_banded"])
def test_plan_counts_match_the_graph(name):
    prob = synth.make(name)
    lam = orc.lambda_structure(prob)[0]
    d = api.schur_plan_host(lam)
    dim = np.asarray(lam.dim)
    is_lm = dim == dim.min()
    assert d["nc"] == int((~is_lm).sum()) and d["nl"] == int(is_lm.sum())
    assert d["no"] == prob.v0.size
    # one block product per pair of observers of a landmark (a <= b): sum over landmarks of k (k + 1) / 2
    lm_of_edge = np.where(is_lm[prob.v0], prob.v0, prob.v1)
    k = np.bincount(lm_of_edge, minlength=dim.size)[is_lm]
    assert d["n_pairs"] == int((k * (k + 1) // 2).sum())
    # S holds every pose's diagonal block and at most every co-observed pair
    assert d["nc"] <= d["n_sblk"] <= d["nc"] * (d["nc"] + 1) // 2
    assert d["n_items"] >= d["n_sblk"] and d["n_multi"] <= d["n_sblk"]


def test_plan_does_not_depend_on_the_thread_count():
    # 100 000 observations: above the size from which the passes are cut among the threads
    a = _plan("ba_medium", 1)
    b = _plan("ba_medium", 4)
    c = _plan("ba_medium", 7)
    assert a == b == c, (a, b, c)


@pytest.mark.parametrize("name,rank,world,sparse", [("ba_small", 0, 1, False), ("ba_interleaved", 0, 1, False),
                                                   ("ba_medium", 1, 2, False), ("ba_banded", 1, 2, True)])
def test_every_pass_cut_among_threads_gives_the_same_plan(name, rank, world, sparse):
    """SPP_PLAN_MIN_WORK=1 cuts every pass (observation scan, camera lists, pair lists by row of S) among the threads
    even on a small graph: more threads than some ranges have columns, the unsorted-observation fallback of the
    interleaved numbering, a landmark shard, and the union pattern of a sharded sparse S"""
    a = _plan(name, 1, rank, world, sparse)
    b = _plan(name, 5, rank, world, sparse, min_work=1)
    c = _plan(name, 16, rank, world, sparse, min_work=1)
    assert a == b == c, (a, b, c)


def test_landmark_shards_partition_the_work():
    full = _plan("ba_medium", 2)
    shards = [_plan("ba_medium", 2, r, 2) for r in range(2)]
    assert sum(s["nl"] for s in shards) == full["nl"] and abs(shards[0]["nl"] - shards[1]["nl"]) <= 1
    assert sum(s["no"] for s in shards) == full["no"]
    assert sum(s["n_pairs"] for s in shards) == full["n_pairs"]
    assert all(s["nc"] == full["nc"] for s in shards)
    # sparse reduced system: every rank holds the UNION block structure (the all-reduced buffer adds like blocks)
    u = [_plan("ba_banded", 2, r, 2, True) for r in range(2)]
    assert u[0]["n_sblk"] == u[1]["n_sblk"] == _plan("ba_banded", 2, 0, 1, True)["n_sblk"]


def test_rejects_bad_input():
    lam = orc.lambda_structure(synth.make("se2_small"))[0]  # one block width: no landmark part
    with pytest.raises(api.SppError):
        api.schur_plan_host(lam)


# ---- the recorded fingerprint ----------------------------------------------------------------------------------------
# Per case: nc, nl, no, n_pairs, n_sblk, n_items, n_multi, checksum (pair lists, block list of S, item records, XCD
# ranges), checksum_all (every list and scalar that the device plan uploads or keeps). Recorded from the plan as it was
# BEFORE schur_plan_host() was split into phases (spp_schur_plan.cpp); a change of the plan's result has to change this
# table on purpose. (The synth cases go through numpy's generator: the same values came out of that earlier build on a
# second machine, so the inputs are portable.) The switches are read once per process, so every environment is a child process that evaluates all
# of its cases.
FINGERPRINT_CHILD = r"""
import sys, json, os
sys.path[:0] = [%r, os.path.join(%r, "tests")]
import numpy as np
from slam_plus_plus_amd import api, synth
from slam_plus_plus_amd.blockcsc import structure_from_pairs
from oracle import spp_oracle as orc
import schur_fixtures as fx
import test_cam_order_host as co

def lam_of(name):
    return orc.lambda_structure(synth.make(name))[0]

def ring(camera_blocks):
    # the smallest closed loop the camera-order rule accepts (tests/test_cam_order_host.py: ring-fifth-6-8); with
    # camera_blocks also a camera-camera block between neighbours of the loop, which the accepted order stores
    # transposed wherever it reverses the two (a_tr = 1 item records)
    nc, dp = 168, 6
    st = co._graph(nc, dp, co._band_pairs(nc, nc // 10, True))[0]
    order, used = api.schur_cam_order_host(st)[:2]
    assert used, "the rule no longer accepts the loop"
    if not camera_blocks:
        return st
    i = np.arange(nc)
    a, b = np.minimum(i, (i + 1) %% nc), np.maximum(i, (i + 1) %% nc)
    st = structure_from_pairs(st.dim, np.concatenate([st.row_idx, a]), np.concatenate([st.col_idx, b]))[0]
    o2, used2 = api.schur_cam_order_host(st)[:2]
    pos = np.empty(nc, np.int64)
    pos[o2] = np.arange(nc)
    assert used2 and np.array_equal(o2, order) and (pos[a] > pos[b]).any(), "no camera-camera block is reversed"
    return st

out = {}
def put(tag, lam, *a, **k):
    d = api.schur_plan_host(lam, *a, **k)
    out[tag] = [d[key] for key in ("nc", "nl", "no", "n_pairs", "n_sblk", "n_items", "n_multi", "checksum", "checksum_all")]

put("ba_small", lam_of("ba_small"))
if sys.argv[1] == "all":
    put("ba_interleaved", lam_of("ba_interleaved"))
    put("lm2d_small", lam_of("lm2d_small"))
    put("ba_medium 1/2", lam_of("ba_medium"), 1, 2)
    banded = lam_of("ba_banded")
    put("ba_banded sparse 1/2", banded, 1, 2, True)
    put("ba_banded sparse", banded, 0, 1, True)
    put("mis66", fx.make("mis66")[0], mis=True)
    put("ring-fifth-6-8", ring(False))
    put("ring-fifth-6-8 + camera blocks", ring(True))
print(json.dumps(out))
"""

RECORDED = {
    '': {   # every switch at its default
        'ba_small': (30, 1500, 7000, 27363, 465, 465, 0, -3483711703387120103, 3715577702227944784),
        'ba_interleaved': (25, 900, 4000, 14635, 325, 325, 0, 2044530526373732354, 4307527839191075599),
        'lm2d_small': (80, 200, 802, 2010, 407, 407, 0, -3576261367263093488, 1432125091731537988),
        'ba_medium 1/2': (150, 10000, 50305, 214529, 5517, 5517, 0, 6976821493733558884, 6692288831176822083),
        'ba_banded sparse 1/2': (600, 15000, 75000, 225000, 7799, 7799, 0, 7833681322732303198, -645211028342656411),
        'ba_banded sparse': (600, 30000, 150000, 450000, 7799, 7799, 0, 4482660595254495377, -5375373520449042219),
        'mis66': (22, 2120, 4239, 6358, 43, 46, 3, 6792182602900669238, -5361852305462679958),
        'ring-fifth-6-8': (168, 2688, 5376, 8064, 2856, 2856, 0, -1715555521255416321, 6413900661363926547),
        'ring-fifth-6-8 + camera blocks': (168, 2688, 5376, 8064, 2856, 2856, 0, -5765239483729953131, 5333027880825863054),
    },
    'SPP_SACC_FACTORED=0': {
        'ba_small': (30, 1500, 7000, 27363, 465, 465, 0, 8463305894241590809, -5616273855013661741),
    },
    'SPP_SACC_ULM=0': {
        'ba_small': (30, 1500, 7000, 27363, 465, 465, 0, -3483711703387120103, 3544198973525928305),
    },
    'SPP_SACC_XCD=0': {
        'ba_small': (30, 1500, 7000, 27363, 465, 465, 0, -4663871102261509533, 3526029727418344230),
    },
    'SPP_SACC_TILE_COLS=0': {
        'ba_small': (30, 1500, 7000, 27363, 465, 465, 0, 4922458397623882126, -2765313924536022111),
    },
    'SPP_SACC_TILE=1': {
        'ba_small': (30, 1500, 7000, 27363, 465, 465, 0, 5544147457629794398, -6958558442293214161),
    },
}

THREADS = {"one thread": {"SPP_PLAN_THREADS": "1"}, "five threads, every pass cut": {"SPP_PLAN_THREADS": "5", "SPP_PLAN_MIN_WORK": "1"}}


def _fingerprints(switch, threads):
    import json
    env = {k: v for k, v in os.environ.items() if not k.startswith("SPP_") or k == "SPP_LIB"}
    env.update(THREADS[threads])
    if switch:
        env.update([switch.split("=")])
    r = subprocess.run([sys.executable, "-c", FINGERPRINT_CHILD % (ROOT, ROOT), "one" if switch else "all"], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return {k: tuple(v) for k, v in json.loads(r.stdout.strip().split("\n")[-1]).items()}


@pytest.mark.parametrize("threads", list(THREADS))
@pytest.mark.parametrize("switch", list(RECORDED))
def test_plan_matches_the_recorded_fingerprint(switch, threads):
    got = _fingerprints(switch, threads)
    print(switch or "defaults", threads, got)
    assert set(got) == set(RECORDED[switch])
    for case, want in RECORDED[switch].items():
        assert got[case] == want, (switch, threads, case, got[case], want)
