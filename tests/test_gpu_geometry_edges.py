"""Every linearization and update kernel of spp_geometry.hip against the 50-digit fixture tests/golden/geometry_edges.npz
(tests/geometry_ref.py; coverage, scales and the constants c: tests/test_geometry_ref_host.py): one
launch per family over its whole case list, |kernel - reference| <= c eps scale entry by entry; apply=False; the offset
kernels bit for bit beside the id kernels; and every kernel at n = 1, 255, 256, 257, 65537, each edge bit-identical to the
same edge of the small launch (thread mapping and tails are all that is under test at those sizes)."""
import functools

import numpy as np
import pytest

import geometry_cases as gc
import geometry_mirrors as gm
from slam_plus_plus_amd import api

pytestmark = pytest.mark.gpu
SIZES = [1, 255, 256, 257, 65537]


@functools.lru_cache(maxsize=None)
def _gold():
    return gm.load()


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def _up(ctx, a, dtype=np.float64):
    return api.DeviceArray.from_host(ctx, np.ascontiguousarray(a, dtype=dtype).ravel())


def _linearize(ctx, fn, n, ins, widths):
    """fn(n, *inputs, J0, J1, r) -> {J0, J1, r} as (n, width) arrays; inputs: (array, dtype)"""
    dev = [_up(ctx, a, t) for a, t in ins]
    out = [api.DeviceArray(ctx, max(1, w * n)) for w in widths]
    fn(n, *[d.ptr for d in dev], *[o.ptr for o in out])
    ctx.synchronize()
    res = {k: o.download()[:w * n].reshape(n, w) for k, o, w in zip(("J0", "J1", "r"), out, widths)}
    for d in dev + out:
        d.free()
    return res


# ---- one runner per kernel: (ctx, the fixture, idx) -> outputs of the edges idx (every vertex array as it stands)
def run_se3(ctx, g, idx):
    E = g["se3_edges"][idx]
    return _linearize(ctx, ctx.se3_linearize_device, len(idx), [(E[:, 0], np.int32), (E[:, 1], np.int32), (g["se3_poses"], np.float64),
                                                                (E[:, 2:8], np.float64)], (36, 36, 6))


def run_se3_at(ctx, g, idx):
    E = g["se3_edges"][idx]
    st, _, _ = gm.interleave(g["se3_poses"], g["se3_poses"], 3)          # pose i at offset 9 i
    return _linearize(ctx, ctx.se3_linearize_at_device, len(idx), [(9 * E[:, 0], np.int64), (9 * E[:, 1], np.int64), (st, np.float64),
                                                                   (E[:, 2:8], np.float64)], (36, 36, 6))


def run_se2(ctx, g, idx):
    E = g["se2_edges"][idx]
    return _linearize(ctx, ctx.se2_linearize_device, len(idx), [(E[:, 0], np.int32), (E[:, 1], np.int32), (g["se2_poses"], np.float64),
                                                                (E[:, 2:5], np.float64)], (9, 9, 3))


def run_se2_at(ctx, g, idx):
    E = g["se2_edges"][idx]
    st, _, _ = gm.interleave(g["se2_poses"], g["se2_poses"], 2)          # pose i at offset 5 i
    return _linearize(ctx, ctx.se2_linearize_at_device, len(idx), [(5 * E[:, 0], np.int64), (5 * E[:, 1], np.int64), (st, np.float64),
                                                                   (E[:, 2:5], np.float64)], (9, 9, 3))


def _run_off(fn_name, fam, zw, widths):
    def run(ctx, g, idx):
        o, base = g[fam + "_obs"][idx], gc.offsets(g[fam + "_dim"])
        return _linearize(ctx, getattr(ctx, fn_name), len(idx), [(base[o[:, 0].astype(int)], np.int64), (base[o[:, 1].astype(int)], np.int64),
                                                                 (g[fam + "_state"], np.float64), (o[:, 2:2 + zw], np.float64)], widths)
    return run


run_xyz = _run_off("se3_xyz_linearize_device", "xyz", 3, (18, 9, 3))
run_rb = _run_off("se2_rb_linearize_device", "rb", 2, (6, 4, 2))


def _run_proj(fn_name, fam, widths):
    def run(ctx, g, idx):
        o = g[fam + "_obs"][idx]
        return _linearize(ctx, getattr(ctx, fn_name), len(idx), [(o[:, 0], np.int32), (o[:, 1], np.int32), (g[fam + "_cams"], np.float64),
                                                                 (g[fam + "_intr"], np.float64), (g[fam + "_pts"], np.float64),
                                                                 (o[:, 2:], np.float64)], widths)
    return run


run_ba = _run_proj("ba_linearize_device", "ba", (12, 6, 2))
run_stereo = _run_proj("ba_stereo_linearize_device", "stereo", (18, 9, 3))
KERNELS = {"se3": (run_se3, "se3_edges"), "se3_at": (run_se3_at, "se3_edges"), "xyz": (run_xyz, "xyz_obs"), "ba": (run_ba, "ba_obs"),
           "stereo": (run_stereo, "stereo_obs"), "se2": (run_se2, "se2_edges"), "se2_at": (run_se2_at, "se2_edges"), "rb": (run_rb, "rb_obs")}


@functools.lru_cache(maxsize=None)
def _small(ctx, name):
    """the one launch of a kernel over its whole case list (shared by the tests below, never modified)"""
    run, key = KERNELS[name]
    return run(ctx, _gold(), np.arange(_gold()[key].shape[0]))


def _judge(fam, got, label):
    g = _gold()
    q = gm.quotients(g, fam, got)
    print(label, " ".join("%s %.3g (case %d)" % (k, v.max(), v.argmax()) for k, v in q.items()))
    for k, v in q.items():
        assert np.isfinite(np.asarray(got[k])).all(), (label, k)
        assert (v <= gc.C[fam][k]).all(), (label, k, v.max(), int(v.argmax()), gc.C[fam][k])


@pytest.mark.parametrize("name", ["se3", "xyz", "ba", "stereo", "se2", "rb"])
def test_linearization_matches_the_50_digit_reference(ctx, name):
    """|kernel - reference| / (eps scale) <= c for every entry of J0, J1, r of every case. Measured on the MI355X (largest
    quotient, c in brackets): DESIGN.md section 18 holds the table."""
    _judge(name, _small(ctx, name), name)


@pytest.mark.parametrize("name", ["se3", "se2"])
def test_offset_kernels_give_the_bits_of_the_id_kernels(ctx, name):
    a, b = _small(ctx, name), _small(ctx, name + "_at")
    for k in a:
        assert np.abs(a[k]).max() > 0 and np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", sorted(KERNELS))
def test_every_edge_keeps_its_bits_at_every_launch_size(ctx, name, n):
    run, key = KERNELS[name]
    small = _small(ctx, name)
    ne = _gold()[key].shape[0]
    idx = np.random.default_rng(n).permutation(np.arange(n) % ne) if n > 1 else np.array([ne - 1])
    big = run(ctx, _gold(), idx)
    for k in small:
        assert big[k].shape[0] == n and np.array_equal(big[k], small[k][idx]), (name, n, k)


# ---- updates
def _se3_update(ctx, p, d, apply=True):
    dp, dd = _up(ctx, p), _up(ctx, d)
    nrm = ctx.se3_update_device(p.shape[0], dp.ptr, dd.ptr, apply)
    out = dp.download().reshape(p.shape)
    dp.free(), dd.free()
    return out, nrm


def _slam3d_update(ctx, p, d, apply=True):
    """the poses interleaved with 3-wide landmarks: pose i at offset 9 i"""
    st, dx, _ = gm.interleave(p, d, 3)
    ds, dd, do = _up(ctx, st), _up(ctx, dx), _up(ctx, 9 * np.arange(p.shape[0]), np.int64)
    nrm = ctx.slam3d_update_device(st.size, ds.ptr, dd.ptr, p.shape[0], do.ptr, apply)
    out = ds.download().reshape(-1, 9)
    ds.free(), dd.free(), do.free()
    return out, nrm, st.reshape(-1, 9), dx.reshape(-1, 9)


def _ba_update(ctx, cams, dcam, pts, dpt, apply=True, seed=3):
    """increments scattered over dx in a shuffled order of 6- and 3-wide slots"""
    nc, npt = cams.shape[0], pts.shape[0]
    order = np.random.default_rng(seed).permutation(nc + npt)
    w = np.where(order < nc, 6, 3)
    start = np.concatenate([[0], np.cumsum(w)])[:-1]
    off = np.empty(nc + npt, dtype=np.int64)
    off[order] = start
    dx = np.zeros(max(1, int(w.sum())))
    for i in range(nc):
        dx[off[i]:off[i] + 6] = dcam[i]
    for i in range(npt):
        dx[off[nc + i]:off[nc + i] + 3] = dpt[i]
    dc, dp, dd = _up(ctx, cams if nc else np.zeros(6)), _up(ctx, pts if npt else np.zeros(3)), _up(ctx, dx)
    oc, op = _up(ctx, off[:nc] if nc else np.zeros(1), np.int64), _up(ctx, off[nc:] if npt else np.zeros(1), np.int64)
    nrm = ctx.ba_update_device(nc, dc.ptr, oc.ptr, npt, dp.ptr, op.ptr, dd.ptr, int(w.sum()), apply)
    res = dc.download().reshape(-1, 6)[:nc], dp.download().reshape(-1, 3)[:npt], nrm
    for a in (dc, dp, dd, oc, op):
        a.free()
    return res


def _judge_plus(out, label):
    _judge("plus", {"out": out, "R": gc.rodrigues(out[:, 3:])}, label)


def test_se3_compositions_match_the_50_digit_reference(ctx):
    """se3_update, slam3d_update (poses at offsets 9 i between landmarks, which take the plain sum) and ba_update (cameras;
    increments at shuffled offsets, points the plain sum) on the composition cases; compositions that cross pi are compared
    as rotation matrices. Then apply=False: the state keeps its bits and the norm is the same."""
    g = _gold()
    p, d = g["plus_p"], g["plus_d"]
    out, nrm = _se3_update(ctx, p, d)
    _judge_plus(out, "se3_update")
    same, nrm0 = _se3_update(ctx, p, d, apply=False)
    assert np.array_equal(same, p) and nrm0 == nrm and nrm > 0
    out3, nrm, st, dx = _slam3d_update(ctx, p, d)
    assert np.array_equal(out3[:, :6], out)                      # the same device function behind both
    assert np.array_equal(out3[:, 6:], st[:, 6:] + dx[:, 6:])
    same, nrm0, _, _ = _slam3d_update(ctx, p, d, apply=False)
    assert np.array_equal(same, st) and nrm0 == nrm and nrm > 0
    pts, dpt = st[:, 6:], dx[:, 6:]
    cams, pts2, nrm = _ba_update(ctx, p, d, pts, dpt)
    _judge_plus(cams, "ba_update")
    assert np.array_equal(pts2, pts + dpt)
    c0, p0, nrm0 = _ba_update(ctx, p, d, pts, dpt, apply=False)
    assert np.array_equal(c0, p) and np.array_equal(p0, pts) and nrm0 == nrm and nrm > 0
    # no cameras, no points, nothing at all
    c1, p1, _ = _ba_update(ctx, p[:0], d[:0], pts, dpt)
    assert c1.shape[0] == 0 and np.array_equal(p1, pts + dpt)
    c2, p2, _ = _ba_update(ctx, p, d, pts[:0], dpt[:0])
    assert p2.shape[0] == 0 and np.array_equal(c2, cams)
    assert _ba_update(ctx, p[:0], d[:0], pts[:0], dpt[:0])[2] == 0.0


def _se2_update(ctx, p, d, apply=True):
    dp, dd = _up(ctx, p), _up(ctx, d)
    nrm = ctx.se2_update_device(p.shape[0], dp.ptr, dd.ptr, apply)
    out = dp.download().reshape(p.shape)
    dp.free(), dd.free()
    return out, nrm


def _slam2d_update(ctx, p, d, apply=True):
    """the poses interleaved with 2-wide landmarks: pose i at offset 5 i, its angle at 5 i + 2"""
    st, dx, _ = gm.interleave(p, d, 2)
    ds, dd, do = _up(ctx, st), _up(ctx, dx), _up(ctx, 5 * np.arange(p.shape[0]) + 2, np.int64)
    nrm = ctx.slam2d_update_device(st.size, ds.ptr, dd.ptr, p.shape[0], do.ptr, apply)
    out = ds.download().reshape(-1, 5)
    ds.free(), dd.free(), do.free()
    return out, nrm, st.reshape(-1, 5), dx.reshape(-1, 5)


def test_se2_updates_match_the_50_digit_reference(ctx):
    g = _gold()
    p, d = g["upd2_p"], g["upd2_d"]
    out, nrm = _se2_update(ctx, p, d)
    _judge("upd2", {"out": out}, "se2_update")
    same, nrm0 = _se2_update(ctx, p, d, apply=False)
    assert np.array_equal(same, p) and nrm0 == nrm and nrm > 0
    out2, nrm, st, dx = _slam2d_update(ctx, p, d)
    assert np.array_equal(out2[:, :3], out) and np.array_equal(out2[:, 3:], st[:, 3:] + dx[:, 3:])
    same, nrm0, _, _ = _slam2d_update(ctx, p, d, apply=False)
    assert np.array_equal(same, st) and nrm0 == nrm and nrm > 0


@functools.lru_cache(maxsize=None)
def _small_updates(ctx):
    g = _gold()
    return _se3_update(ctx, g["plus_p"], g["plus_d"])[0], _se2_update(ctx, g["upd2_p"], g["upd2_d"])[0]


@pytest.mark.parametrize("n", SIZES)
def test_every_vertex_keeps_its_bits_at_every_update_size(ctx, n):
    g = _gold()
    s3, s2 = _small_updates(ctx)
    rng = np.random.default_rng(n)
    i3, i2 = rng.permutation(np.arange(n) % s3.shape[0]), rng.permutation(np.arange(n) % s2.shape[0])
    p, d = g["plus_p"][i3], g["plus_d"][i3]
    assert np.array_equal(_se3_update(ctx, p, d)[0], s3[i3])
    assert np.array_equal(_slam3d_update(ctx, p, d)[0][:, :6], s3[i3])
    rows = np.random.default_rng(n + 1).normal(size=(n, 3))
    cams, pts, _ = _ba_update(ctx, p, d, rows, rows[::-1], seed=n)
    assert np.array_equal(cams, s3[i3]) and np.array_equal(pts, rows + rows[::-1])
    p, d = g["upd2_p"][i2], g["upd2_d"][i2]
    assert np.array_equal(_se2_update(ctx, p, d)[0], s2[i2])
    assert np.array_equal(_slam2d_update(ctx, p, d)[0][:, :3], s2[i2])
