"""Time the multi-group assembly against the two one-group assemblies of its parts, and the resident Gauss-Newton
iteration, on a victoria-park-shaped synthetic graph (6969 poses, 151 landmarks, about 3600 observations).

    python tools/slam2d_time.py [--reps 50] [--warmup 5]

Each figure is the median over --reps calls of the hipEvent time the library records around one assembly
(SPP_FLAG_PROFILE, phase "assemble"), after --warmup calls; the two one-group assemblies run through
spp_assemble_analyze / spp_assemble_device, which exist unchanged before the multi-group entry points did. Prints one
JSON line. DESIGN.md section 14 says whether a result has been recorded."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from slam_plus_plus_amd import api, nonlinear, synth  # noqa: E402
from slam_plus_plus_amd.formats import slam2d_linearize  # noqa: E402


def _timed(ctx, call, reps, warmup):
    for _ in range(warmup):
        call()
    ms = []
    for _ in range(reps):
        call()
        ms.append(ctx.phase_ms()["assemble"])
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    p = synth.slam2d_problem(6969, 151, 7, name="victoria_shape", views=(16, 32), window=60)
    groups = slam2d_linearize(p.dim, p.state, p.odo, p.odo_info, p.obs, p.obs_info)
    ctx = api.Context(0, api.FLAG_PROFILE)
    up = lambda x: api.DeviceArray.from_host(ctx, np.ascontiguousarray(x).ravel())
    dev = [[up(g[k]) for k in ("J0", "J1", "Om", "r")] for g in groups]
    out = {"poses": int((p.dim == 3).sum()), "landmarks": int((p.dim == 2).sum()), "odometry_edges": int(groups[0].v0.size),
           "observations": int(groups[1].v0.size)}
    # the parts, each alone through the one-group entry points (a part's Lambda has the same vertices)
    for key, g, d in (("odometry_alone_ms", groups[0], dev[0]), ("observations_alone_ms", groups[1], dev[1])):
        st = ctx.assemble_analyze(_dims_of(p.dim, g), *_edges_of(p.dim, g), g.d0, g.d1, g.rd, -1)
        dv, de = api.DeviceArray(ctx, st.nvals), api.DeviceArray(ctx, st.n)
        out[key], out[key.replace("_ms", "_min_ms")] = _timed(
            ctx, lambda: ctx.assemble_device(d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, 0.0, dv.ptr, de.ptr), a.reps, a.warmup)
    st = ctx.assemble_analyze_groups(p.dim, [(g.v0, g.v1, g.d0, g.d1, g.rd) for g in groups], [p.odo_seq, p.obs_seq], 0)
    dv, de = api.DeviceArray(ctx, st.nvals), api.DeviceArray(ctx, st.n)
    ptrs = [[d4[k].ptr for d4 in dev] for k in range(4)]
    out["groups_ms"], out["groups_min_ms"] = _timed(
        ctx, lambda: ctx.assemble_groups_device(*ptrs, 0.0, dv.ptr, de.ptr), a.reps, a.warmup)
    out["sum_of_parts_ms"] = out["odometry_alone_ms"] + out["observations_alone_ms"]
    deg = np.bincount(np.concatenate([g.v0 for g in groups] + [g.v1 for g in groups]), minlength=p.dim.size)
    # computed here from the vertex degrees by the library's rule (degree <= 24: sequential kernel), not read from a trace
    out["launches_groups_computed"] = 2 + sum(int(((p.dim == w) & (deg <= 24)).any()) + int(((p.dim == w) & (deg > 24)).any()) for w in (3, 2))
    ctx.close()
    # resident Gauss-Newton: wall time per iteration (each ends with the 8-byte norm on the host), first iteration apart
    path = nonlinear._ResidentSlam2DPath()
    path.begin(nonlinear.CSlam2D.from_problem(p))
    t = []
    for _ in range(6):
        t0 = time.perf_counter()
        ok, norm = path.step()
        path.apply()
        t.append(1e3 * (time.perf_counter() - t0))
    out["gn_first_iteration_ms"], out["gn_iteration_ms"] = t[0], float(np.median(t[1:]))
    path.close()
    print(json.dumps(out))


def _dims_of(dim, g):
    """a part alone only accepts the widths of its own shape: the observations keep every vertex (3 and 2), the odometry
    runs over the poses renumbered 0 .. n_poses - 1"""
    return dim if g.d0 != g.d1 else dim[dim == g.d0]


def _edges_of(dim, g):
    if g.d0 != g.d1:
        return g.v0, g.v1
    new_id = np.cumsum(dim == g.d0) - 1
    return new_id[g.v0], new_id[g.v1]


if __name__ == "__main__":
    main()
