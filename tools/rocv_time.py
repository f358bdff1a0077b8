"""Time the resident Gauss-Newton iteration of a range-only constant-velocity graph in both solver modes: 2000 receivers, 8
transmitters, 6 ranges per receiver (synth.rocv_problem).

    python tools/rocv_time.py [--receivers 2000] [--transmitters 8] [--ranges 6] [--iterations 5]

MODE_AUTO would take the Schur mode for the widths {6, 3}: it eliminates the 8 transmitters and leaves a dense reduced system
over all receivers; the sparse mode sees a chain with a few dense columns ordered last. Per iteration the hipEvent times the
library records (SPP_FLAG_PROFILE) around the assembly and around the factorization + solve are added -- the linearization
and the update are the same kernels in both modes --, and the wall time of the whole step is taken beside them; the first
iteration (symbolic analysis, allocations) is reported apart, the figures are medians over --iterations further ones, both
modes in one run. Prints one JSON line. DESIGN.md section 22 says whether a result has been recorded."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from slam_plus_plus_amd import api, nonlinear, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--receivers", type=int, default=2000)
    ap.add_argument("--transmitters", type=int, default=8)
    ap.add_argument("--ranges", type=int, default=6)
    ap.add_argument("--iterations", type=int, default=5)
    a = ap.parse_args()
    p = synth.rocv_problem(a.receivers, a.transmitters, 85, n_ranges=a.ranges, name="rocv_time")
    out = {"receivers": a.receivers, "transmitters": a.transmitters, "ranges": int(p.rng.shape[0]), "iterations": a.iterations}
    for key, mode in (("sparse", api.MODE_SPARSE), ("schur", api.MODE_SCHUR)):
        path = nonlinear._ResidentROCVPath(0, mode=mode)
        path.ctx.set_profiling(True)
        path.begin(nonlinear.CRocv.from_problem(p))
        ev, wall, norms = [], [], []
        for _ in range(1 + a.iterations):
            t0 = time.perf_counter()
            path.linearize()
            path.assemble()
            ms = path.ctx.phase_ms()["assemble"]
            path._analyze_once()
            if path.ctx.factor_solve_device(path.d_vals.ptr, path.d_eta.ptr) != 0:
                sys.exit("not positive definite in mode " + key)
            ms += path.ctx.phase_ms()["total"]
            norms.append(path._update(True))
            wall.append(1e3 * (time.perf_counter() - t0))
            ev.append(ms)
        out[key] = {"mode": path.ctx.info("MODE"), "first_event_ms": ev[0], "event_ms": float(np.median(ev[1:])),
                    "event_min_ms": float(np.min(ev[1:])), "first_wall_ms": wall[0], "wall_ms": float(np.median(wall[1:])),
                    "dx_norms": [float("%.4g" % n) for n in norms]}
        path.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
