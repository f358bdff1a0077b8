"""GPU: the camera order of a closed loop at the other pose widths -- 7-wide cameras (loop73: 330
cameras, 19 tile rows) and 3-wide poses (loop32: 300 poses, 8 tile rows), the rings of tests/schur_fixtures.py. The arc
length is 128 / gcd(128, dp) cameras: 64 for the 6-wide loop of tests/test_gpu_cam_order.py, 128 for both widths here, so
arc A is cameras 0..127, arc B the next 128 that do not see them and everything else the separators. Camera-camera blocks
occur in both senses (the reversed ones are added transposed), and the S block that is split over several work items
belongs to a reversed pair: s_multi_kernel<7> / <3> sums it, and adds its camera-camera block, in reversed position
(tests/test_schur_fixtures_73_host.py asserts these conditions on the host).

The tests are those of tests/test_gpu_cam_order.py, whose helpers they use: S | rhs entry by entry against the longdouble
reference in the reported order; x with SPP_SCHUR_CAM_ORDER 1 and 0 in child processes; two shards with pack / sum /
unpack; a non-positive pivot in arc B and in the separators."""
import numpy as np
import pytest

import schur_fixtures as fx
import schur_fixtures_73 as fx73
import schur_ref
import test_gpu_cam_order as base
from slam_plus_plus_amd import api

pytestmark = pytest.mark.gpu
LOOPS = [("loop73", 7, fx73.LOOP73_SPLIT), ("loop32", 3, fx.LOOP32_SPLIT)]
IDS = [c[0] for c in LOOPS]


def _nc(lam):
    return int((lam.dim == lam.dim.max()).sum())


@pytest.mark.parametrize("kind,dp,split", LOOPS, ids=IDS)
def test_schur_form_in_the_camera_order_matches_the_reference(kind, dp, split):
    lam, eta = base.system(kind)
    nc = _nc(lam)
    c = api.Context(0)
    c.analyze(lam, api.MODE_SCHUR)
    assert c.info("N_POSES") == nc and c.info("N_REDUCED") == nc * dp
    order = c.ordering(lam.nb)[:nc]
    assert not np.array_equal(order, np.arange(nc)), "the loop's camera order was not accepted"
    host_order, used, natural, chosen = api.schur_cam_order_host(lam)
    assert used and np.array_equal(host_order, order), "ctx.ordering() reports the order the host rule chooses"
    pos = np.empty(nc, np.int64)
    pos[order] = np.arange(nc)
    u, v = fx.ring_a_edges(nc)
    assert (pos[u] > pos[v]).any() and (pos[u] < pos[v]).any(), "camera-camera blocks in both senses"
    assert pos[split[0]] > pos[split[1]], "the split S block is not reversed"
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
    P = base._ref_in_order(lam, eta, order, kind)
    assert P.dp == dp and P.has_A[min(pos[list(split)]), max(pos[list(split)])], "the split pair's camera-camera block"
    ratio = schur_ref.check_schur_buffer(P, bufs[0], False, c.info("S_LD"))   # (entries outside the upper blocks: exactly 0.0)
    print("%s, camera order %s -> %s: largest error / bound of S | rhs %.3f" % (kind, natural, chosen, ratio))
    dr.upload(eta)
    assert c.factor_solve_device(dv.ptr, dr.ptr) == 0
    print("%s: landmark / pose part, error / bound: %s" % (kind, schur_ref.check_solution(P, lam, eta, dr.download())))
    for d in (dv, dr, dS):
        d.free()
    c.close()


@pytest.mark.parametrize("kind,dp,split", LOOPS, ids=IDS)
def test_solution_with_the_order_on_and_off(kind, dp, split, tmp_path):
    """both sides within the bound of schur_ref.check_solution, each bit-reproducible (asserted by the helper); not
    bit-identical to each other"""
    lam, eta = base.system(kind)
    nc = _nc(lam)
    on, x_on = base._solve_in_child(kind, "1", tmp_path)
    off, x_off = base._solve_in_child(kind, "0", tmp_path)
    assert off["order"] == list(range(nc)) and on["order"] != off["order"]
    assert on["streamed"] > 0 and off["streamed"] > 0, "the streamed dense factor did not run"
    for d, x in ((on, x_on), (off, x_off)):
        P = base._ref_in_order(lam, eta, np.asarray(d["order"]), kind)
        print("%s, order %s: landmark / pose part, error / bound: %s" % (kind, "on" if d is on else "off",
                                                                         schur_ref.check_solution(P, lam, eta, x)))


@pytest.mark.parametrize("kind,dp,split", LOOPS, ids=IDS)
def test_two_shards_with_the_packed_exchange(kind, dp, split):
    lam, eta = base.system(kind)
    nc = _nc(lam)
    ctxs, bufs = [], []
    for rank in range(2):
        c = api.Context(0)
        c.set_shard(rank, 2)
        c.analyze(lam, api.MODE_SCHUR)
        dv, dr = api.DeviceArray.from_host(c, lam.vals), api.DeviceArray.from_host(c, eta)
        dS, dP = api.DeviceArray(c, c.schur_buffer_size()), api.DeviceArray(c, c.schur_packed_size())
        c.schur_form(dv.ptr, dr.ptr, dS.ptr)
        c.schur_pack(dS.ptr, dP.ptr)
        c.synchronize()
        ctxs.append(c)
        bufs.append((dv, dr, dS, dP))
    orders = [c.ordering(lam.nb)[:nc] for c in ctxs]
    assert np.array_equal(orders[0], orders[1]) and not np.array_equal(orders[0], np.arange(nc)), "every rank chooses the same order"
    psum = sum(b[3].download() for b in bufs)
    x = np.zeros_like(eta)
    is_lm = lam.dim == lam.dim.min()
    lms = np.flatnonzero(is_lm)
    for r, (c, (dv, dr, dS, dP)) in enumerate(zip(ctxs, bufs)):
        dP.upload(psum)
        c.schur_unpack(dP.ptr, dS.ptr)
        assert c.schur_finish(dv.ptr, dS.ptr, dr.ptr) == 0
        c.synchronize()
        xr = dr.download()
        mine = np.concatenate([np.flatnonzero(~is_lm)] * (r == 0) + [lms[r::2]])   # (landmarks are dealt round-robin)
        idx = schur_ref.pose_index(lam, mine)
        x[idx] = xr[idx]
    P = base._ref_in_order(lam, eta, orders[0], kind)
    print("%s, two shards: landmark / pose part, error / bound: %s" % (kind, schur_ref.check_solution(P, lam, eta, x)))
    for c, b in zip(ctxs, bufs):
        for d in b:
            d.free()
        c.close()


@pytest.mark.parametrize("where", ["arc B", "separator"])
@pytest.mark.parametrize("kind,dp,split", LOOPS, ids=IDS)
def test_a_late_pivot_is_reported_and_the_context_recovers(kind, dp, split, where):
    lam, eta = base.system(kind)
    order = api.schur_cam_order_host(lam)[0]
    sep = int(np.flatnonzero(np.diff(order) < 0)[-1]) + 1   # (natural order inside the parts: the last drop opens the separators)
    cam = int(order[sep - 10]) if where == "arc B" else int(order[sep + 10])   # (arc B ends where the separators start)
    vals = lam.vals.copy()
    p = lam.col_ptr[cam + 1] - 1   # (cameras come first: the diagonal block closes the column)
    assert lam.row_idx[p] == cam and lam.dim[cam] == dp
    D = vals[lam.blk_off[p]:lam.blk_off[p] + dp * dp].reshape(dp, dp)
    D -= 10.0 * np.abs(D).max() * np.eye(dp)
    solver = api.CLinearSolver_HIP(mode=api.MODE_SCHUR)
    x = eta.copy()
    assert solver.Solve_PosDef_Blocky(lam.with_vals(vals), x) is False
    assert np.array_equal(x, eta)
    assert solver.Solve_PosDef_Blocky(lam, x)
    assert np.linalg.norm(lam.matvec(x) - eta) / np.linalg.norm(eta) < 1e-11
