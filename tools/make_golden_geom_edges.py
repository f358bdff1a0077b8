"""tests/golden/geometry_edges.npz: the inputs of tests/geometry_cases.py, the 50-digit reference outputs of
tests/geometry_ref.py for them (rounded once to float64) and, per case, the branch every threshold of
slam_plus_plus_amd/csrc/spp_geometry.hip takes, decided in mpmath from the inputs. Host only: numpy + mpmath.

    python tools/make_golden_geom_edges.py          # rewrites the fixture

tests/test_geometry_ref_host.py calls generate() and requires equality with the committed file.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import geometry_cases as gc   # noqa: E402
import geometry_ref as gr     # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "geometry_edges.npz")


def _stack(rows):
    return [np.array(c) for c in zip(*rows)]


def generate():
    g = gc.inputs()
    # SE(3) pose-pose edges
    P, E = g["se3_poses"], g["se3_edges"]
    out = _stack([gr.se3_edge(P[int(e[0])], P[int(e[1])], e[2:8]) for e in E])
    g["se3_J0"], g["se3_J1"], g["se3_r"], g["se3_aux"], g["se3_br"] = out
    g["se3_br_cols"] = np.array(gr.SE3_BR)
    # pose-landmark XYZ edges
    x, base, obs = g["xyz_state"], gc.offsets(g["xyz_dim"]), g["xyz_obs"]
    out = _stack([gr.xyz_edge(x[base[int(o[0])]:base[int(o[0])] + 6], x[base[int(o[1])]:base[int(o[1])] + 3], o[2:5]) for o in obs])
    g["xyz_J0"], g["xyz_J1"], g["xyz_r"], g["xyz_br"] = out
    g["xyz_br_cols"] = np.array(gr.XYZ_BR)
    # mono and stereo projections
    for fam, fn, cols in (("ba", gr.ba_edge, gr.BA_BR), ("stereo", gr.stereo_edge, gr.STEREO_BR)):
        cams, intr, pts, obs = (g[fam + k] for k in ("_cams", "_intr", "_pts", "_obs"))
        out = _stack([fn(cams[int(o[0])], intr[int(o[0])], pts[int(o[1])], o[2:]) for o in obs])
        g[fam + "_J0"], g[fam + "_J1"], g[fam + "_r"], g[fam + "_aux"], g[fam + "_br"] = out
        g[fam + "_br_cols"] = np.array(cols)
    # 2D pose-pose edges
    P, E = g["se2_poses"], g["se2_edges"]
    out = _stack([gr.se2_edge(P[int(e[0])], P[int(e[1])], e[2:5]) for e in E])
    g["se2_J0"], g["se2_J1"], g["se2_r"], g["se2_br"] = out
    g["se2_br_cols"] = np.array(gr.SE2_BR)
    # range-bearing edges
    x, base, obs = g["rb_state"], gc.offsets(g["rb_dim"]), g["rb_obs"]
    out = _stack([gr.rb_edge(x[base[int(o[0])]:base[int(o[0])] + 3], x[base[int(o[1])]:base[int(o[1])] + 2], o[2:4]) for o in obs])
    g["rb_J0"], g["rb_J1"], g["rb_r"], g["rb_aux"], g["rb_br"] = out
    g["rb_br_cols"] = np.array(gr.RB_BR)
    # x (+) dx on SE(3) and SE(2)
    out = _stack([gr.plus_case(p, d) for p, d in zip(g["plus_p"], g["plus_d"])])
    g["plus_out"], g["plus_R"], g["plus_aux"], g["plus_br"] = out
    g["plus_br_cols"] = np.array(gr.PLUS_BR)
    g["upd2_out"] = np.array([gr.upd2_case(p, d) for p, d in zip(g["upd2_p"], g["upd2_d"])])
    for k in list(g):
        if k.endswith("_br"):
            g[k] = g[k].astype(np.int8)
    return g


if __name__ == "__main__":
    g = generate()
    np.savez_compressed(PATH, **g)
    print("%s: %d arrays, %d bytes" % (PATH, len(g), os.path.getsize(PATH)))
    for k in sorted(g):
        if k.endswith("_br"):
            print(k, g[k].shape)
