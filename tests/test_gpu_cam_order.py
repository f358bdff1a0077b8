"""GPU: the dense Schur path under the camera order of a closed loop (schur_cam_order in spp_schur_plan.cpp, DESIGN
section 12) on 300-camera loops (15 tile rows, co-visibility +-36 cameras: a band of 3 tiles, arcs of 3 and 6 tile rows
exist) -- the smallest shape with two independent arcs at tile granularity.

S | rhs entry by entry against the longdouble reference of tests/schur_ref.py, mapped through ctx.ordering(), with
camera-camera blocks whose cameras the order reverses (they are added transposed); x with SPP_SCHUR_CAM_ORDER 1 and 0 in
child processes: both within the reference's bound, each bit-reproducible -- NOT bit-identical to each other, the factor
sums in another order; two shards with pack / sum / unpack; a non-positive pivot in arc B and in the separator; an open
chain keeps the natural order and its bits."""
import copy
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import schur_fixtures as fx
import schur_fixtures_73 as fx73
import schur_ref
from slam_plus_plus_amd import api, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NC = 300
SPLIT, SPLIT_PTS = (21, 26), 2100
_CACHE = {}


def system(kind):
    """'loop': the ring of synth.ba_problem plus camera-camera edges (c, c + 5) for every 7th camera; 'chain': the same
    without the points whose window wraps around (no camera-camera edges); a name of schur_fixtures_73.SHAPES or
    schur_fixtures.SHAPES: that fixture (the loops of the other widths)"""
    if kind in _CACHE:
        return _CACHE[kind]
    if kind in fx73.SHAPES or kind in fx.SHAPES:   # the loops of other widths (tests/test_gpu_cam_order_73.py)
        _CACHE[kind] = fx73.make_any(kind)
        return _CACHE[kind]
    prob = synth.ba_problem(NC, 4000, 16000, 5, heavy_tail=False, spread=0.06)
    cam, pt = prob.v0.astype(np.int64), prob.v1.astype(np.int64) - NC
    if kind == "chain":
        lo, hi = np.full(prob.npts, NC), np.zeros(prob.npts, np.int64)
        np.minimum.at(lo, pt, cam)
        np.maximum.at(hi, pt, cam)
        keep_pt = hi - lo <= 2 * 18 + 1
        new_id = np.cumsum(keep_pt) - 1
        sel = keep_pt[pt]
        cam, pt = cam[sel], new_id[pt[sel]]
    else:
        sel = np.ones(cam.size, bool)
    npts = int(pt.max()) + 1
    J0 = prob.J0[sel].reshape(-1, 6, 2).transpose(0, 2, 1)
    J1 = prob.J1[sel].reshape(-1, 3, 2).transpose(0, 2, 1)
    s = 1.0 / np.abs(J1).max()   # (pixels -> O(1): the conditioning of the landmark blocks is what the fixtures assume)
    groups = [(cam, NC + pt, s * J0, s * J1, s * prob.r[sel])]
    if kind == "loop":
        rng = np.random.default_rng(7)
        u = np.arange(0, NC - 5, 7)
        groups.append((u, u + 5, 0.5 * rng.standard_normal((u.size, 6, 6)), 0.5 * rng.standard_normal((u.size, 6, 6)),
                       rng.standard_normal((u.size, 6))))
        # SPLIT_PTS more points seen by cameras SPLIT = (21, 26) alone: their S block has more than 2048 block products,
        # so it is split over several work items and summed by s_multi_kernel -- and the order reverses the two cameras
        # (21 ends up in the separators, 26 in an arc: asserted below), so that kernel adds the (21, 26) block transposed
        extra = npts + np.arange(SPLIT_PTS)
        npts += SPLIT_PTS
        for c in SPLIT:
            groups.append((np.full(SPLIT_PTS, c), NC + extra, rng.standard_normal((SPLIT_PTS, 3, 6)),
                           np.eye(3)[None] + 0.25 * rng.standard_normal((SPLIT_PTS, 3, 3)), rng.standard_normal((SPLIT_PTS, 3))))
    dim = np.array([6] * NC + [3] * npts, np.int32)
    _CACHE[kind] = fx.build_system(dim, groups, 1.0, 0)
    return _CACHE[kind]


def _ref_in_order(lam, eta, order_blocks, kind="loop"):
    """the reference of the whole system `kind` with the poses at the positions the library reports"""
    key = "ref" if kind == "loop" else "ref " + kind
    if key not in _CACHE:
        _CACHE[key] = schur_ref.schur_ref(lam, eta, schur_ref.guided_elim(lam))
    R = _CACHE[key]
    nat = np.searchsorted(R.poses, order_blocks)
    assert np.array_equal(R.poses[nat], order_blocks)
    dp, nc = R.dp, nat.size
    e = (nat[:, None] * dp + np.arange(dp)[None, :]).ravel()
    P = copy.copy(R)
    P.poses = np.asarray(order_blocks)
    P.S, P.M, P.rhs, P.Mrhs = R.S[np.ix_(e, e)], R.M[np.ix_(e, e)], R.rhs[e], R.Mrhs[e]
    P.k, P.k_all, P.obs_count = R.k[np.ix_(nat, nat)], R.k_all[np.ix_(nat, nat)], R.obs_count[nat]
    P.has_A = np.triu((R.has_A | R.has_A.T)[np.ix_(nat, nat)])
    pos = np.empty(nc, np.int64)
    pos[nat] = np.arange(nc)
    P.obs_pose = pos[R.obs_pose]
    i1, i2 = np.nonzero(np.triu(P.k_all > 0) | P.has_A)
    o = np.lexsort((i1, i2))
    P.pattern = list(zip(i1[o].tolist(), i2[o].tolist()))
    return P


def test_schur_form_in_the_camera_order_matches_the_reference():
    lam, eta = system("loop")
    c = api.Context(0)
    c.analyze(lam, api.MODE_SCHUR)
    order = c.ordering(lam.nb)[:NC]
    assert not np.array_equal(order, np.arange(NC)), "the loop's camera order was not accepted"
    host_order, used, natural, chosen = api.schur_cam_order_host(lam)
    assert used and np.array_equal(host_order, order), "ctx.ordering() reports the order the host rule chooses"
    pos = np.empty(NC, np.int64)
    pos[order] = np.arange(NC)
    u = np.arange(0, NC - 5, 7)
    assert (pos[u] > pos[u + 5]).any() and (pos[u] < pos[u + 5]).any(), "camera-camera blocks in both senses"
    assert SPLIT[0] in u and pos[SPLIT[0]] > pos[SPLIT[1]], "the camera-camera block of the split S block is not reversed"
    assert api.schur_plan_host(lam)["n_multi"] >= 1, "no S block is split over several work items"
    dv, dr = api.DeviceArray.from_host(c, lam.vals), api.DeviceArray.from_host(c, eta)
    dS = api.DeviceArray(c, c.schur_buffer_size())
    bufs = []
    for _ in range(2):
        dS.upload(np.full(dS.n, np.nan))
        c.schur_form(dv.ptr, dr.ptr, dS.ptr)
        c.synchronize()
        bufs.append(dS.download())
    assert np.array_equal(bufs[0], bufs[1]), "S | rhs not bit-reproducible"
    P = _ref_in_order(lam, eta, order)
    ratio = schur_ref.check_schur_buffer(P, bufs[0], False, c.info("S_LD"))   # (entries outside the upper blocks: exactly 0.0)
    print("loop, camera order %s -> %s: largest error / bound of S | rhs %.3f" % (natural, chosen, ratio))
    # and the solution of the same context
    dr.upload(eta)
    assert c.factor_solve_device(dv.ptr, dr.ptr) == 0
    schur_ref.check_solution(P, lam, eta, dr.download())
    for d in (dv, dr, dS):
        d.free()
    c.close()


CHILD = r"""
import sys, json, hashlib
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import test_gpu_cam_order as t
from slam_plus_plus_amd import api
lam, eta = t.system(sys.argv[1])
c = api.Context(0)
c.analyze(lam, api.MODE_SCHUR)
dv, dr = api.DeviceArray.from_host(c, lam.vals), api.DeviceArray(c, lam.n)
xs = []
for _ in range(2):
    dr.upload(eta)
    assert c.factor_solve_device(dv.ptr, dr.ptr) == 0
    xs.append(dr.download())
np.save(sys.argv[2], xs[0])
print(json.dumps({"sha": [hashlib.sha256(x.tobytes()).hexdigest() for x in xs], "order": c.ordering(lam.nb)[:c.info("N_POSES")].tolist(),
                  "streamed": c.info("DENSE_STREAMED")}))
"""


def _solve_in_child(kind, switch, tmp_path):
    out = str(tmp_path / ("x_%s_%s.npy" % (kind, switch)))
    env = dict(os.environ, SPP_SCHUR_CAM_ORDER=switch)
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests")), kind, out], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    d = json.loads(r.stdout.strip().split("\n")[-1])
    assert d["sha"][0] == d["sha"][1], "x not bit-reproducible with SPP_SCHUR_CAM_ORDER=%s" % switch
    return d, np.load(out)


def test_solution_with_the_order_on_and_off(tmp_path):
    """both sides within the bound of schur_ref.check_solution against the reference. They are NOT bit-identical: the
    factor of the reordered S sums in another order (only their agreement through the reference is asserted)"""
    lam, eta = system("loop")
    on, x_on = _solve_in_child("loop", "1", tmp_path)
    off, x_off = _solve_in_child("loop", "0", tmp_path)
    assert off["order"] == list(range(NC)) and on["order"] != off["order"]
    assert on["streamed"] > 0 and off["streamed"] > 0, "the streamed dense factor did not run"
    for d, x in ((on, x_on), (off, x_off)):
        P = _ref_in_order(lam, eta, np.asarray(d["order"]))
        print("order %s: landmark / pose part, error / bound: %s" % ("on" if d is on else "off", schur_ref.check_solution(P, lam, eta, x)))
    print("on against off: relative difference %.3e" % (np.linalg.norm(x_on - x_off) / np.linalg.norm(x_off)))


def test_an_open_chain_keeps_the_natural_order_and_its_bits(tmp_path):
    on, _ = _solve_in_child("chain", "1", tmp_path)
    off, _ = _solve_in_child("chain", "0", tmp_path)
    assert on["order"] == off["order"] == list(range(NC))
    assert on["sha"] == off["sha"]


def test_two_shards_with_the_packed_exchange():
    lam, eta = system("loop")
    ctxs, bufs = [], []
    for rank in range(2):
        c = api.Context(0)
        c.set_shard(rank, 2)
        c.analyze(lam, api.MODE_SCHUR)
        dv, dr = api.DeviceArray.from_host(c, lam.vals), api.DeviceArray.from_host(c, eta)
        dS = api.DeviceArray(c, c.schur_buffer_size())
        c.schur_form(dv.ptr, dr.ptr, dS.ptr)
        c.synchronize()
        ctxs.append(c)
        bufs.append((dv, dr, dS))
    orders = [c.ordering(lam.nb)[:NC] for c in ctxs]
    assert np.array_equal(orders[0], orders[1]) and not np.array_equal(orders[0], np.arange(NC)), "every rank chooses the same order"
    packed = []
    for c, (dv, dr, dS) in zip(ctxs, bufs):
        dP = api.DeviceArray(c, c.schur_packed_size())
        c.schur_pack(dS.ptr, dP.ptr)
        c.synchronize()
        packed.append(dP)
    psum = sum(p.download() for p in packed)
    x = np.zeros_like(eta)
    is_lm = lam.dim == 3
    lms = np.flatnonzero(is_lm)
    for r, (c, (dv, dr, dS), dP) in enumerate(zip(ctxs, bufs, packed)):
        dP.upload(psum)
        c.schur_unpack(dP.ptr, dS.ptr)
        assert c.schur_finish(dv.ptr, dS.ptr, dr.ptr) == 0
        c.synchronize()
        xr = dr.download()
        mine = np.concatenate([np.flatnonzero(~is_lm)] * (r == 0) + [lms[r::2]])   # (landmarks are dealt round-robin)
        idx = schur_ref.pose_index(lam, mine)
        x[idx] = xr[idx]
    P = _ref_in_order(lam, eta, orders[0])
    print("two shards: landmark / pose part, error / bound: %s" % (schur_ref.check_solution(P, lam, eta, x),))
    for c, arrs, dP in zip(ctxs, bufs, packed):
        for d in arrs + (dP,):
            d.free()
        c.close()


@pytest.mark.parametrize("where", ["arc B", "separator"])
def test_a_late_pivot_is_reported_and_the_context_recovers(where):
    lam, eta = system("loop")
    order = api.schur_cam_order_host(lam)[0]
    sep = int(np.flatnonzero(np.diff(order) < 0)[-1]) + 1   # (natural order inside the parts: the last drop opens the separators)
    cam = int(order[sep - 10]) if where == "arc B" else int(order[sep + 10])   # (arc B ends where the separators start)
    vals = lam.vals.copy()
    p = lam.col_ptr[cam + 1] - 1   # (cameras come first: the diagonal block closes the column)
    assert lam.row_idx[p] == cam
    D = vals[lam.blk_off[p]:lam.blk_off[p] + 36].reshape(6, 6)
    D -= 10.0 * np.abs(D).max() * np.eye(6)
    solver = api.CLinearSolver_HIP(mode=api.MODE_SCHUR)
    x = eta.copy()
    assert solver.Solve_PosDef_Blocky(lam.with_vals(vals), x) is False
    assert np.array_equal(x, eta)
    assert solver.Solve_PosDef_Blocky(lam, x)
    assert np.linalg.norm(lam.matvec(x) - eta) / np.linalg.norm(eta) < 1e-11
