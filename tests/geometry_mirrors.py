"""The float64 mirrors of slam_plus_plus_amd/formats.py run over the geometry fixture (tests/golden/geometry_edges.npz),
their outputs named like the fixture's reference outputs, and the quotient |a - reference| / (eps scale) both the host test
(mirrors) and the GPU test (kernels) are judged by. numpy / scipy only."""
import os

import numpy as np

import geometry_cases as gc
from slam_plus_plus_amd import formats

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geometry_edges.npz")
OUTPUTS = {"se3": ("J0", "J1", "r"), "xyz": ("J0", "J1", "r"), "ba": ("J0", "J1", "r"), "stereo": ("J0", "J1", "r"),
           "se2": ("J0", "J1", "r"), "rb": ("J0", "J1", "r"), "plus": ("out", "R"), "upd2": ("out",)}


def load():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


def br(g, fam, col):
    """one column of a family's branch table, by name"""
    return g[fam + "_br"][:, list(g[fam + "_br_cols"]).index(col)].astype(int)


def pi_crossing(g):
    """the composition cases whose product of canonical quaternions has w < 0: compared as rotation matrices"""
    return br(g, "plus", "w_neg") == 1


def mirrors(g):
    """{family: {output: array}} of formats.py on the fixture's inputs"""
    m = {}
    ne = g["se3_edges"].shape[0]
    p = formats.se3_linearize(g["se3_poses"], g["se3_edges"], np.tile(np.eye(6), (ne, 1, 1)))
    m["se3"] = {"J0": p.J0, "J1": p.J1, "r": p.r}
    k = g["xyz_obs"].shape[0]
    _, p = formats.slam3d_linearize(g["xyz_dim"], g["xyz_state"], np.zeros((0, 8)), np.zeros((0, 6, 6)), g["xyz_obs"],
                                    np.tile(np.eye(3), (k, 1, 1)))
    m["xyz"] = {"J0": p.J0, "J1": p.J1, "r": p.r}
    p = formats.ba_linearize(g["ba_cams"], g["ba_intr"], g["ba_pts"], g["ba_obs"])
    m["ba"] = {"J0": p.J0, "J1": p.J1, "r": p.r}
    p = formats.stereo_linearize(g["stereo_cams"], g["stereo_intr"], g["stereo_pts"], g["stereo_obs"])
    m["stereo"] = {"J0": p.J0, "J1": p.J1, "r": p.r}
    ne = g["se2_edges"].shape[0]
    p = formats.se2_linearize(g["se2_poses"], g["se2_edges"], np.tile(np.eye(3), (ne, 1, 1)))
    m["se2"] = {"J0": p.J0, "J1": p.J1, "r": p.r}
    # the same edges through slam2d_linearize's odometry group (poses only: vertex i at offset 3 i)
    p2, _ = formats.slam2d_linearize(np.full(g["se2_poses"].shape[0], 3), g["se2_poses"].ravel(), g["se2_edges"],
                                     np.tile(np.eye(3), (ne, 1, 1)), np.zeros((0, 4)), np.zeros((0, 2, 2)))
    m["se2_slam2d"] = {"J0": p2.J0, "J1": p2.J1, "r": p2.r}
    k = g["rb_obs"].shape[0]
    _, p = formats.slam2d_linearize(g["rb_dim"], g["rb_state"], np.zeros((0, 5)), np.zeros((0, 3, 3)), g["rb_obs"],
                                    np.tile(np.eye(2), (k, 1, 1)))
    m["rb"] = {"J0": p.J0, "J1": p.J1, "r": p.r}
    out = formats.se3_plus(g["plus_p"], g["plus_d"])
    m["plus"] = {"out": out, "R": gc.rodrigues(out[:, 3:])}
    # slam3d_plus on the same poses interleaved with 3-wide landmarks (plain sums)
    st, dx, dim = interleave(g["plus_p"], g["plus_d"], 3)
    o3 = formats.slam3d_plus(dim, st, dx)
    m["plus_slam3d"] = {"out": o3.reshape(-1, 9)[:, :6], "R": gc.rodrigues(o3.reshape(-1, 9)[:, 3:6]), "lm": o3.reshape(-1, 9)[:, 6:]}
    return m


def interleave(p, d, w):
    """flat state and increment: every pose (row of p) followed by a w-wide landmark, so that no pose after the first sits at
    a multiple of its width; returns state, dx, dim"""
    n, pw = p.shape
    rng = np.random.default_rng(7)
    st = np.concatenate([p, rng.normal(size=(n, w))], axis=1).ravel()
    dx = np.concatenate([d, rng.normal(size=(n, w))], axis=1).ravel()
    return st, dx, np.tile(np.array([pw, w], dtype=np.int32), n)


def quotients(g, fam, got, scales=None):
    """{output: (n,) the largest |got - reference| / (eps scale) of each case}. The rotation part of a composition that
    crosses pi is judged as a matrix (output "R") and left out of "out"; every other case is judged as a vector, too."""
    scales = gc.SCALES[fam](g) if scales is None else scales
    q = {}
    for name in OUTPUTS[fam]:
        ref, a = g[fam + "_" + name], np.asarray(got[name]).reshape(g[fam + "_" + name].shape)
        e = np.abs(a - ref) / (gc.EPS * scales[name])
        if fam == "plus" and name == "out":
            e[pi_crossing(g), 3:] = 0
        q[name] = e.max(axis=1)
    return q
