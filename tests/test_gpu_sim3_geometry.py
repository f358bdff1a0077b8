"""spp_sim3_ba_linearize_device / spp_sim3_update_device on the device: the Sim(3) projection edge and the camera update
Log(Exp(cam) Exp(d)) against the 50-digit golden (tests/golden/sim3_edges.npz, tests/sim3_ref.py) within C eps scale
(tests/sim3_cases.py: scales from the inputs, C from the float64 mirror's own error), every cell of (|s|, |w|) and of the
kernel's own evaluation; launch sizes of both; apply = False; empty camera and point sets."""
import functools
import os

import numpy as np
import pytest

from slam_plus_plus_amd import api
import sim3_cases as sc

pytestmark = pytest.mark.gpu
EDGES = os.path.join(os.path.dirname(__file__), "golden", "sim3_edges.npz")


@functools.lru_cache(maxsize=None)
def gold():
    return dict(np.load(EDGES))


def run_linearize(ctx, cams, intr, pts, obs):
    n = obs.shape[0]
    up = lambda a: api.DeviceArray.from_host(ctx, np.ascontiguousarray(a).ravel())
    out = [api.DeviceArray(ctx, w * n) for w in (14, 6, 2)]
    for o in out:
        o.upload(np.full(o.n, np.nan))
    ctx.sim3_ba_linearize_device(n, up(obs[:, 0].astype(np.int32)).ptr, up(obs[:, 1].astype(np.int32)).ptr, up(cams).ptr,
                                 up(intr).ptr, up(pts).ptr, up(obs[:, 2:4]).ptr, *[o.ptr for o in out])
    ctx.synchronize()
    return [o.download().reshape(n, -1) for o in out]


def run_update(ctx, v, d, seed, apply=True):
    """v (+) d through spp_sim3_update_device: camera i at a shuffled offset of a dx that also holds three points"""
    n = v.shape[0]
    rng = np.random.default_rng(seed)
    off = 7 * rng.permutation(n).astype(np.int64)
    dx = np.empty(7 * n + 9)
    dx[off[:, None] + np.arange(7)] = d
    dpt = rng.normal(size=(3, 3))
    dx[7 * n:] = dpt.ravel()
    pts = rng.normal(size=(3, 3))
    up = lambda a: api.DeviceArray.from_host(ctx, np.ascontiguousarray(a).ravel())
    d_v, d_p = up(v), up(pts)
    nrm = ctx.sim3_update_device(n, d_v.ptr, up(off).ptr, 3, d_p.ptr, up(7 * n + 3 * np.arange(3, dtype=np.int64)).ptr,
                                 up(dx).ptr, dx.size, apply=apply)
    return d_v.download().reshape(n, 7), d_p.download().reshape(3, 3), pts, dpt, nrm, dx


@functools.lru_cache(maxsize=None)
def base_output():
    g = gold()
    ctx = api.Context(0)
    lin = run_linearize(ctx, g["cams"], g["intr"], g["pts"], g["obs"])
    upd = run_update(ctx, g["upd_v"], g["upd_d"], 0)
    ctx.close()
    return lin, upd


def test_linearize_against_the_50_digit_golden():
    g = gold()
    (J0, J1, r), _ = base_output()
    s = sc.edge_scales(g["cams"], g["intr"], g["pts"], g["obs"], g["aux"])
    assert all(np.isfinite(a).all() for a in (J0, J1, r))               # the point on the axis included
    for k, got in (("J0", J0), ("J1", J1), ("r", r)):
        err, bound = np.abs(got - g[k]), sc.C[k] * sc.EPS * s[k]
        print(k, "largest kernel quotient |kernel - reference| / (eps scale): %.4f (C = %d)" % ((err / (sc.EPS * s[k])).max(), sc.C[k]))
        assert (err <= bound).all(), (k, (err / bound).max())
    assert not J0[:, 12:].any()                                         # the scale column: exact zeros
    on_axis = int(np.flatnonzero(g["branches"][:, 3])[0])
    assert np.array_equal(r[on_axis], g["obs"][on_axis, 2:4] - g["intr"][int(g["obs"][on_axis, 0]), 2:4])


def test_update_against_the_50_digit_golden():
    g = gold()
    _, (out, pts_out, pts, dpt, nrm, dx) = base_output()
    us = sc.update_scales(g["upd_v"], g["upd_d"], g["upd_aux"])
    assert np.isfinite(out).all()
    far = np.abs(np.pi - g["upd_aux"][:, 0]) > 3e-3                     # across pi the axis flips: compared as rotation matrices
    flipped = ~far & (np.einsum("ei,ei->e", out[:, 3:6], g["upd_out"][:, 3:6]) < 0)
    assert flipped.sum() <= 1 and (~far).sum() == 2
    cols = np.ones(out.shape, dtype=bool)
    cols[flipped, 3:6] = False
    err = np.abs(out - g["upd_out"])
    print("out: largest kernel quotient %.4f (C = %d)" % ((err / (sc.EPS * us["out"]))[cols].max(), sc.C["out"]))
    assert (err <= sc.C["out"] * sc.EPS * us["out"])[cols].all()
    errR = np.abs(sc.rodrigues(out[:, 3:6]) - g["upd_R"])
    print("R: largest kernel quotient %.4f (C = %d)" % ((errR / (sc.EPS * us["R"])).max(), sc.C["R"]))
    assert (errR <= sc.C["R"] * sc.EPS * us["R"]).all()
    assert np.array_equal(pts_out, pts + dpt)                           # points: plain sums
    assert abs(nrm - np.linalg.norm(dx)) <= 8 * sc.EPS * np.linalg.norm(dx) * np.log2(dx.size)


def test_apply_false_and_empty_sets():
    g = gold()
    _, (_, _, _, _, nrm, _) = base_output()
    ctx = api.Context(0)
    out, pts_out, pts, _, nrm0, dx = run_update(ctx, g["upd_v"], g["upd_d"], 0, apply=False)
    assert np.array_equal(out, g["upd_v"]) and np.array_equal(pts_out, pts) and nrm0 == nrm
    up = lambda a: api.DeviceArray.from_host(ctx, np.ascontiguousarray(a).ravel())
    d_dx = up(dx)
    # no cameras: the points alone move; no points: the cameras alone; neither: the norm alone
    d_p = up(pts)
    n1 = ctx.sim3_update_device(0, None, None, 3, d_p.ptr, up(3 * np.arange(3, dtype=np.int64)).ptr, d_dx.ptr, dx.size)
    assert np.array_equal(d_p.download().reshape(3, 3), pts + dx[:9].reshape(3, 3)) and n1 == nrm
    v = g["upd_v"][:5]
    d_v = up(v)
    n2 = ctx.sim3_update_device(5, d_v.ptr, up(7 * np.arange(5, dtype=np.int64)).ptr, 0, None, None, d_dx.ptr, dx.size)
    small = run_update(ctx, v, dx[:35].reshape(5, 7), 3)[0]
    assert np.array_equal(d_v.download().reshape(5, 7), small) and n2 == nrm
    assert ctx.sim3_update_device(0, None, None, 0, None, None, d_dx.ptr, dx.size) == nrm
    assert ctx.sim3_update_device(0, None, None, 0, None, None, d_dx.ptr, 0) == 0.0
    ctx.close()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 65537])
def test_launch_sizes(n):
    """n observations / n cameras drawn from the cases in a shuffled order: every row bit-identical to the case it copies"""
    g = gold()
    (lin, upd) = base_output()
    src = np.random.default_rng(n).permutation(np.arange(n) % g["obs"].shape[0])
    ctx = api.Context(0)
    out = run_linearize(ctx, g["cams"], g["intr"], g["pts"], g["obs"][src])
    for a, b in zip(out, lin):
        assert np.array_equal(a, b[src])
    src = np.random.default_rng(n + 1).permutation(np.arange(n) % g["upd_v"].shape[0])
    got = run_update(ctx, g["upd_v"][src], g["upd_d"][src], n + 2)[0]
    ctx.close()
    assert np.array_equal(got, upd[0][src])
