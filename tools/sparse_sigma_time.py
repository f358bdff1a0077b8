"""Time the selected inversion on the kept SPARSE factor against the solve route it replaces, on the two pose-graph
shapes (sphere2500, manhattan3500), in one process.

    python tools/sparse_sigma_time.py [--reps 20] [--warmup 3] [--shape SHAPE] [--out profiles/NAME.json]

Per shape Lambda is assembled on the device as bench.py assembles it and analyzed in SPP_MODE_SPARSE. Then, each a
hipEvent time (torch.cuda.Event on the stream the context is bound to; the stream is drained before the first event),
median / min / max of --reps runs after --warmup:
  factor_solve_ms   one spp_factor_solve_device (the call that leaves the factor);
  sigma_ms          one spp_sparse_sigma_device: every block of Sigma on the pattern of Lambda;
  solve_route_ms    what gave every pose's covariance before: ceil(n / 128) passes of spp_sparse_solve_device with k = 128 on
                    one n x 128 panel (the time of the solves alone: building the unit columns and reading the blocks out
                    of n x n doubles are left out, in the route's favour);
  launches          kernel launches of one spp_sparse_sigma_device (from the front table).
The gate DESIGN.md section 29 states is sigma_over_solve_route < 1 on both shapes. Prints one JSON line and, with --out,
writes it to that file."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from slam_plus_plus_amd import api, synth  # noqa: E402

SHAPES = ("sphere2500", "manhattan3500")
PASS = 128


def _stats(t):
    return {"median": float(np.median(t)), "min": float(np.min(t)), "max": float(np.max(t)), "runs": len(t)}


def launches(fr):
    """per level: update columns and pivot columns of the fronts of classes 0 - 2, the same two and the mirror of classes
    3 - 4 (the update columns only where a front of the level has a parent); the gather"""
    n = 1
    for lvl in set(int(l) for l in fr["level"]):
        at = fr["level"] == lvl
        for big in (False, True):
            g = at & ((fr["cls"] >= 3) == big)
            if np.any(g):
                n += (2 if big else 1) + int(np.any(fr["parent"][g] >= 0))
    return n


def measure(shape, reps, warmup, torch, stream):
    prob = synth.make(shape)
    ctx = api.Context(0)
    ctx.set_stream(stream.cuda_stream)
    st = ctx.assemble_analyze(prob.dim, prob.v0, prob.v1, prob.d0, prob.d1, prob.rd, prob.unary_vertex)
    d_in = [api.DeviceArray.from_host(ctx, a.ravel()) for a in (prob.J0, prob.J1, prob.Om, prob.r)]
    d_vals, d_eta, d_rhs = api.DeviceArray(ctx, st.nvals), api.DeviceArray(ctx, st.n), api.DeviceArray(ctx, st.n)
    ctx.assemble_device(d_in[0].ptr, d_in[1].ptr, d_in[2].ptr, d_in[3].ptr, prob.damping, d_vals.ptr, d_eta.ptr)
    ctx.synchronize()
    ctx.analyze(st, api.MODE_SPARSE)
    n = int(ctx.info("N"))
    out = {"poses": int(st.nb), "n": n, "nvals": int(st.nvals), "supernodes": int(ctx.info("N_SUPERNODES")),
           "levels": int(ctx.info("N_LEVELS")), "launches": launches(ctx.sparse_fronts()), "passes_of_128": (n + PASS - 1) // PASS}

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
        assert ctx.factor_solve_device(d_vals.ptr, d_rhs.ptr) == 0

    def timed_factor():   # the copy of eta and its drain in front of the first event: only the call is timed
        d_rhs.copy_from(d_eta)
        return timed(factor)

    out["factor_solve_ms"] = _stats([timed_factor() for _ in range(warmup + reps)][warmup:])
    d_rhs.copy_from(d_eta)
    factor()
    assert ctx.info("SPARSE_FACTOR_KEPT") == 1
    d_sigma = api.DeviceArray(ctx, st.nvals)
    out["sigma_ms"] = run(lambda: ctx.sparse_sigma_device(d_sigma.ptr))
    sigma = d_sigma.download()
    # (not a test: the diagonal blocks of three poses against the marginals call, so that a timing of wrong results shows)
    col_ptr, blk_off, dim = np.asarray(st.col_ptr), np.asarray(st.blk_off), np.asarray(st.dim)
    worst = 0.0
    for v in (0, st.nb // 2, st.nb - 1):
        d = int(dim[v])
        p = int(col_ptr[v + 1]) - 1
        blk = sigma[blk_off[p]:blk_off[p] + d * d].reshape((d, d), order="F")
        cov = ctx.sparse_marginals([v])
        worst = max(worst, float(np.linalg.norm(blk - cov) / np.linalg.norm(cov)))
    out["diagonal_blocks_vs_marginals"] = worst
    # the route it replaces, on a zero panel: the time of a pass does not depend on the values
    passes = (n + PASS - 1) // PASS
    dB = api.DeviceArray(ctx, n * PASS)
    E = np.zeros((n, PASS), order="F")

    def solve_route():
        for _ in range(passes):
            ctx.sparse_solve_device(dB.ptr, PASS)

    dB.upload(E.ravel(order="F"))
    out["solve_route_ms"] = run(solve_route)
    out["sigma_over_solve_route"] = out["sigma_ms"]["median"] / out["solve_route_ms"]["median"]
    out["sigma_over_factor_solve"] = out["sigma_ms"]["median"] / out["factor_solve_ms"]["median"]
    for d in d_in + [d_vals, d_eta, d_rhs, d_sigma, dB]:
        d.free()
    ctx.set_stream(None)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", default=None, choices=SHAPES, help="one shape only (a kernel trace of one shape)")
    a = ap.parse_args()
    assert a.reps >= 20, "medians of at least 20 runs"
    import torch
    torch.cuda.init()   # before the library opens the device (as bench.py does)
    stream = torch.cuda.Stream()
    res = {shape: measure(shape, a.reps, a.warmup, torch, stream) for shape in ([a.shape] if a.shape else SHAPES)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
