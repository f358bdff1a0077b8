"""Time the covariance blocks on Lambda's pattern from the kept dense Schur factor against the solve route they replace,
on the Venice-871 shape (871 cameras, 530 304 points, 2 838 740 observations), in one process.

    python tools/schur_sigma_time.py [--reps 20] [--warmup 3] [--out profiles/NAME.json] [--once]

The resident path (nonlinear._ResidentBAPath) linearizes and assembles Lambda on the device once. Then, each a hipEvent
time (torch.cuda.Event on the stream the context is bound to; the stream is drained before the first event), median /
min / max of --reps runs after --warmup:
  factor_solve_ms   one spp_factor_solve_device (the call that leaves the factor);
  sigma_ms          one spp_schur_sigma_device: every stored block of Sigma -- cameras, points, observations;
  sigma_dense_ms    its first step alone, Z = S^-1 (spp_schur_sigma_dense_device);
  solve_route_ms    what gave the CAMERAS' covariances alone before: ceil(n_red / 128) passes of spp_solve_device with
                    k = 128 on a zeroed n x 128 panel (the time of the solves alone: building the unit columns and reading
                    the blocks out are left out, in the route's favour).
The gate DESIGN.md section 33 states is sigma_over_solve_route < 1. --once: after the warm-up one spp_schur_sigma_device
and nothing else (the run a kernel trace is taken of). Prints one JSON line and, with --out, writes it to that file."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from slam_plus_plus_amd import api, nonlinear, synth  # noqa: E402

PASS = 128


def _stats(t):
    return {"median": float(np.median(t)), "min": float(np.min(t)), "max": float(np.max(t)), "runs": len(t)}


def measure(reps, warmup, once):
    import torch
    torch.cuda.init()   # before the library opens the device (as bench.py does)
    s = synth.ba_states(synth.make("venice871"))
    nc = s["cams"].shape[0]
    intr = np.tile(np.array([500.0, 505.0, 320.0, 240.0, 0.0]), (nc, 1))
    obs = np.concatenate([np.stack([s["cam_of"], s["pt_of"]], axis=1).astype(np.float64), s["meas"]], axis=1)
    system = nonlinear.CBundleAdjustment(s["cams"], intr, s["points"], obs)
    path = nonlinear._ResidentBAPath()
    stream = torch.cuda.Stream()
    path.ctx.set_stream(stream.cuda_stream)
    path.begin(system)
    path.linearize()
    alpha = 1e-3 * path.max_hessian_diag()
    path.chi2()
    path._assemble(alpha)
    path._analyze_once()
    ctx = path.ctx
    n, n_red, nvals = int(ctx.info("N")), int(ctx.info("N_REDUCED")), int(ctx.info("NVALS"))
    blocks = (n_red + PASS - 1) // PASS
    out = {"cameras": nc, "points": int(s["points"].shape[0]), "observations": int(obs.shape[0]), "n": n, "n_reduced": n_red,
           "nvals": nvals, "block_rows": blocks, "launches": 3 * blocks - 2 + 3, "passes_of_128": blocks}

    def timed(f):
        stream.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        f()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    def run(f):
        return _stats([timed(f) for _ in range(warmup + reps)][warmup:])

    def factor():
        path.d_dx.copy_from(path.d_eta)
        stream.synchronize()
        assert ctx.factor_solve_device(path.d_vals.ptr, path.d_dx.ptr) == 0

    d_sigma = api.DeviceArray(ctx, nvals)
    if once:
        factor()
        for _ in range(warmup):
            ctx.schur_sigma_device(path.d_vals.ptr, d_sigma.ptr)
        out["sigma_ms"] = _stats([timed(lambda: ctx.schur_sigma_device(path.d_vals.ptr, d_sigma.ptr))])
    else:
        out["factor_solve_ms"] = run(factor)
        factor()
        assert ctx.info("FACTOR_KEPT") == 1
        out["sigma_ms"] = run(lambda: ctx.schur_sigma_device(path.d_vals.ptr, d_sigma.ptr))
        out["sigma_dense_ms"] = run(lambda: ctx._check(ctx.lib.spp_schur_sigma_dense_device(ctx.h)))
        assert ctx.info("FACTOR_KEPT") == 1
        sigma = d_sigma.download()
        # (not a test: the diagonal blocks of two cameras and two points against the marginals call, so that a timing of
        # wrong results shows)
        st = path.st
        col_ptr, blk_off, dim = np.asarray(st.col_ptr), np.asarray(st.blk_off), np.asarray(st.dim)
        cams, lms = np.flatnonzero(dim == dim.max()), np.flatnonzero(dim == dim.min())
        worst = 0.0
        for v in (cams[0], cams[-1], lms[0], lms[-1]):
            d = int(dim[v])
            p = int(col_ptr[v + 1]) - 1
            blk = sigma[blk_off[p]:blk_off[p] + d * d].reshape((d, d), order="F")
            cov = ctx.marginals(path.d_vals.ptr, [int(v)])
            worst = max(worst, float(np.linalg.norm(blk - cov) / np.linalg.norm(cov)))
        out["diagonal_blocks_vs_marginals"] = worst
        out["sigma_all_finite"] = bool(np.all(np.isfinite(sigma)))
        # the route it replaces, for the cameras alone, on a zero panel: the time of a pass does not depend on the values
        dB = api.DeviceArray.from_host(ctx, np.zeros(n * PASS))

        def solve_route():
            for _ in range(blocks):
                ctx.solve_device(path.d_vals.ptr, dB.ptr, PASS)

        out["solve_route_ms"] = run(solve_route)
        dB.free()
        out["sigma_over_solve_route"] = out["sigma_ms"]["median"] / out["solve_route_ms"]["median"]
        out["sigma_over_factor_solve"] = out["sigma_ms"]["median"] / out["factor_solve_ms"]["median"]
    d_sigma.free()
    path.ctx.set_stream(None)
    path.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    assert a.reps >= 20, "medians of at least 20 runs"
    line = json.dumps(measure(a.reps, a.warmup, a.once))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
