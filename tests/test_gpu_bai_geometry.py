"""spp_ba_intrinsics_linearize_device / spp_ba_intrinsics_update_device on the device: the ternary edge CEdgeP2CI3D against
the 50-digit golden (tests/golden/bai_edges.npz, tests/bai_ref.py) within C eps scale, J0 / J1 / r bit for bit those of
spp_ba_linearize_device, the inert column, launch sizes of both, and CVertexIntrinsics::Operator_Plus as written."""
import functools
import os

import numpy as np
import pytest

from slam_plus_plus_amd import api, formats
import bai_cases as bc

pytestmark = pytest.mark.gpu
EDGES = os.path.join(os.path.dirname(__file__), "golden", "bai_edges.npz")


@functools.lru_cache(maxsize=None)
def gold():
    return dict(np.load(EDGES))


def run_kernel(ctx, cams, intr, pts, obs):
    n = obs.shape[0]
    up = lambda a: api.DeviceArray.from_host(ctx, np.ascontiguousarray(a).ravel())
    out = [api.DeviceArray(ctx, w * n) for w in (12, 6, 12, 2)]
    for o in out:
        o.upload(np.full(o.n, np.nan))
    ctx.ba_intrinsics_linearize_device(n, *[up(obs[:, i].astype(np.int32)).ptr for i in range(3)], up(cams).ptr, up(intr).ptr,
                                       up(pts).ptr, up(obs[:, 3:5]).ptr, *[o.ptr for o in out])
    ctx.synchronize()
    return [o.download().reshape(n, -1) for o in out]


@functools.lru_cache(maxsize=None)
def base_output():
    g = gold()
    ctx = api.Context(0)
    out = run_kernel(ctx, g["cams"], g["intr"], g["pts"], g["obs"])
    ctx.close()
    return out


def test_kernel_against_the_50_digit_golden():
    g = gold()
    J0, J1, J2, r = base_output()
    s = bc.edge_scales(g["cams"], g["intr"], g["pts"], g["obs"], g["aux"])
    assert all(np.isfinite(a).all() for a in (J0, J1, J2, r))          # the point on the axis included
    for k, got in (("J0", J0), ("J1", J1), ("J2", J2), ("r", r)):
        err, bound = np.abs(got - g[k]), bc.C[k] * bc.EPS * s[k]
        q = (err[bound > 0] / bound[bound > 0]).max()
        print(k, "largest error / (C eps scale): %.4f" % q)
        assert (err <= bound).all(), (k, q)
    assert not J2[:, 10:].any()                                         # the inert column: exact zeros
    assert np.array_equal(J2[:, 4:8], np.tile([1.0, 0.0, 0.0, 1.0], (J2.shape[0], 1)))
    on_axis = int(np.flatnonzero(g["branches"][:, 2])[0])
    assert not J2[on_axis, [0, 1, 2, 3, 8, 9]].any()


def test_camera_point_and_residual_are_those_of_the_mono_kernel():
    """J0, J1, r bit-identical to spp_ba_linearize_device given the intrinsics each observation uses (one camera row per
    observation: a camera of the cases is seen through several intrinsics vertices)"""
    g = gold()
    J0, J1, _, r = base_output()
    obs = g["obs"]
    n = obs.shape[0]
    co, po, io = (obs[:, i].astype(int) for i in range(3))
    ctx = api.Context(0)
    up = lambda a: api.DeviceArray.from_host(ctx, np.ascontiguousarray(a).ravel())
    out = [api.DeviceArray(ctx, w * n) for w in (12, 6, 2)]
    ctx.ba_linearize_device(n, up(np.arange(n, dtype=np.int32)).ptr, up(po.astype(np.int32)).ptr, up(g["cams"][co]).ptr,
                            up(g["intr"][io]).ptr, up(g["pts"]).ptr, up(obs[:, 3:5]).ptr, *[o.ptr for o in out])
    ctx.synchronize()
    m0, m1, mr = [o.download().reshape(n, -1) for o in out]
    ctx.close()
    assert np.array_equal(m0, J0) and np.array_equal(m1, J1) and np.array_equal(mr, r)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 65537])
def test_launch_sizes(n):
    """n observations drawn from the cases in a shuffled order: every row bit-identical to the case it copies"""
    g = gold()
    base = base_output()
    src = np.random.default_rng(n).permutation(np.arange(n) % g["obs"].shape[0])
    ctx = api.Context(0)
    out = run_kernel(ctx, g["cams"], g["intr"], g["pts"], g["obs"][src])
    ctx.close()
    for a, b in zip(out, base):
        assert np.array_equal(a, b[src])


def test_intrinsics_update():
    """against the 50-digit Operator_Plus to 4 eps relative; the norm runs over the live coordinates only; apply=False
    leaves the state alone and returns the same norm"""
    g = gold()
    v, d, want = g["upd_v"], g["upd_d"], g["upd_out"]
    ni = v.shape[0]
    rng = np.random.default_rng(1)
    off = np.array([3, 40, 12, 27], dtype=np.int64)                   # 6 entries each in a padded dx, anywhere
    dx = rng.normal(size=50)                                           # other vertices' entries and the inert ones: not counted
    for i in range(ni):
        dx[off[i]:off[i] + 5] = d[i]
    ctx = api.Context(0)
    up = lambda a: api.DeviceArray.from_host(ctx, np.ascontiguousarray(a).ravel())
    d_v, d_off, d_dx = up(v), up(off), up(dx)
    n0 = ctx.ba_intrinsics_update_device(ni, d_v.ptr, d_off.ptr, d_dx.ptr, apply=False)
    assert np.array_equal(d_v.download().reshape(ni, 5), v)
    n1 = ctx.ba_intrinsics_update_device(ni, d_v.ptr, d_off.ptr, d_dx.ptr, apply=True)
    got = d_v.download().reshape(ni, 5)
    ctx.close()
    assert n0 == n1 and abs(n0 - np.linalg.norm(d)) <= 4 * bc.EPS * np.linalg.norm(d) * 5
    assert np.all(np.abs(got - want) <= 4 * bc.EPS * np.abs(want)), np.abs(got - want).max()
    assert np.all(np.abs(got - formats.bai_intrinsics_plus(v, d)) <= 4 * bc.EPS * np.abs(want))
    assert np.array_equal(got[3], v[3])                                # a zero increment: kappa / den * den' with den' = den


def _apply_intrinsics_update(ctx, v, d, seed):
    """v (+) d through spp_ba_intrinsics_update_device, vertex i at a shuffled offset 6 j of a padded dx"""
    ni = v.shape[0]
    off = 6 * np.random.default_rng(seed).permutation(ni).astype(np.int64)
    dx = np.full(6 * ni, 1e3)                                          # the inert entries: never read
    dx[off[:, None] + np.arange(5)] = d
    up = lambda a: api.DeviceArray.from_host(ctx, np.ascontiguousarray(a).ravel())
    d_v = up(v)
    ctx.ba_intrinsics_update_device(ni, d_v.ptr, up(off).ptr, up(dx).ptr, apply=True)
    return d_v.download().reshape(ni, 5)


@pytest.mark.parametrize("ni", [1, 255, 256, 257])
def test_every_intrinsics_vertex_keeps_its_bits_at_every_update_size(ni):
    """ni vertices drawn from the four golden update cases in a shuffled order: every row bit-identical to the same case
    in the four-vertex launch (one workgroup, a full one, a tail of one thread)"""
    g = gold()
    ctx = api.Context(0)
    small = _apply_intrinsics_update(ctx, g["upd_v"], g["upd_d"], 0)
    src = np.random.default_rng(ni).permutation(np.arange(ni) % g["upd_v"].shape[0])
    got = _apply_intrinsics_update(ctx, g["upd_v"][src], g["upd_d"][src], ni + 1)
    ctx.close()
    assert np.all(np.abs(small - g["upd_out"]) <= 4 * bc.EPS * np.abs(g["upd_out"]))   # the four-vertex launch is the golden's
    assert np.array_equal(got, small[src])
