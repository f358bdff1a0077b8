"""Time the three calls on the kept factor of a sparse reduced system against the factor-and-solve
they spare, on two shapes analyzed in MODE_SCHUR_SPARSE, in one process:

    python tools/schur_sparse_again_time.py [--reps 20] [--warmup 3] [--shapes ba_banded,synthetic10k] [--out profiles/NAME.json]

  ba_banded      600 cameras, 30 000 points, 150 000 observations: a trajectory, banded reduced system
  synthetic10k   10 000 cameras, 2 000 000 points, 10 000 000 observations (BASELINE config 5)

Lambda is assembled on the device from the graph (spp_assemble_analyze / spp_assemble_device, as bench.py does). Then, each a
hipEvent time (torch.cuda.Event on the stream the context is bound to; the stream is drained before the first event), median
/ min / max of --reps runs after --warmup:
  factor_solve_ms      one spp_factor_solve_device (the call that leaves the factor);
  solve_ms             one spp_schur_sparse_solve_device with k = 1, 6 and 128 columns;
  marginals_ms         one spp_schur_sparse_marginals_device of 20 cameras spread over the trajectory (120 columns; the call
                       drains the stream once on entry, so its host side is inside the time);
  sigma_ms             one spp_schur_sparse_sigma_device: every stored block of Sigma -- cameras, points, observations;
  sigma_inverse_ms     its first step alone: the blocks of Z = S^-1 on S's pattern (spp_schur_sparse_sigma_inverse_device).
`launches` counts the kernel launches of each call from the front table. `columns_times_factor_solve_ms` is what the same
blocks cost without the kept factor: one factor-and-solve per unit column, n x factor_solve_ms. Prints one JSON line per
shape and, with --out, writes them to that file."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from slam_plus_plus_amd import api, synth  # noqa: E402

PASS = 128


def _stats(t):
    return {"median": float(np.median(t)), "min": float(np.min(t)), "max": float(np.max(t)), "runs": len(t)}


def _launches(fr, n_red, nl, no):
    """kernel launches per call, from the front table: the substitutions and the selected inversion go level by level, the
    fronts of classes 0 - 2 and those of classes 3 - 4 of a level in launches of their own"""
    lo, hi = fr["cls"] <= 2, fr["cls"] >= 3
    upd = fr["h"] - 1 - fr["w"] > 0
    solve = inv = 0
    for l in np.unique(fr["level"]):
        at = fr["level"] == l
        solve += 2 * (int(np.any(at & lo)) + int(np.any(at & hi)))           # forward and backward
        inv += int(np.any(at & lo & upd)) + int(np.any(at & lo))              # update columns, pivot columns
        inv += 3 * int(np.any(at & hi & upd)) + 2 * int(np.any(at & hi))      # fetch, columns, mirror | columns, mirror
    inv += 1                                                                  # the gather
    per_pass = solve + 2 + int(nl > 0) + 2 * int(n_red > 0) + int(nl > 0 and no > 0)
    return {"solve_per_pass_of_128": per_pass, "sigma_inverse": inv, "sigma": inv + int(no > 0) + int(nl > 0) + 1}


def measure(shape, reps, warmup):
    import torch
    torch.cuda.init()   # before the library opens the device (as bench.py does)
    prob = synth.make(shape)
    ctx = api.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    st = ctx.assemble_analyze(prob.dim, prob.v0, prob.v1, prob.d0, prob.d1, prob.rd, prob.unary_vertex)
    d_in = [api.DeviceArray.from_host(ctx, a.ravel()) for a in (prob.J0, prob.J1, prob.Om, prob.r)]
    d_vals, d_eta, d_rhs = api.DeviceArray(ctx, st.nvals), api.DeviceArray(ctx, st.n), api.DeviceArray(ctx, st.n)
    ctx.assemble_device(d_in[0].ptr, d_in[1].ptr, d_in[2].ptr, d_in[3].ptr, prob.damping, d_vals.ptr, d_eta.ptr)
    ctx.synchronize()
    ctx.analyze(st, api.MODE_SCHUR_SPARSE)
    assert ctx.info("MODE") == api.MODE_SCHUR_SPARSE
    n, n_red, nvals = int(ctx.info("N")), int(ctx.info("N_REDUCED")), int(ctx.info("NVALS"))
    fr = ctx.sparse_fronts()
    out = {"shape": shape, "cameras": int(ctx.info("N_POSES")), "points": int(ctx.info("N_LANDMARKS")),
           "observations": int(ctx.info("N_OBS")), "n": n, "n_reduced": n_red, "nvals": nvals, "s_blocks": int(ctx.info("S_NNZB")),
           "fronts": int(fr["h"].size), "levels": int(ctx.info("N_LEVELS")), "fronts_per_class": np.bincount(fr["cls"], minlength=5).tolist(),
           "launches": _launches(fr, n_red, int(ctx.info("N_LANDMARKS")), int(ctx.info("N_OBS")))}

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
        d_rhs.copy_from(d_eta)
        stream.synchronize()
        assert ctx.factor_solve_device(d_vals.ptr, d_rhs.ptr) == 0

    out["factor_solve_ms"] = run(factor)
    factor()
    assert ctx.info("SCHUR_SPARSE_FACTOR_KEPT") == 1
    x = d_rhs.download()
    dB = api.DeviceArray.from_host(ctx, np.zeros(n * PASS))   # (the time of a pass does not depend on the values)
    out["solve_ms"] = {}
    for k in (1, 6, PASS):
        out["solve_ms"][str(k)] = run(lambda: ctx.schur_sparse_solve_device(d_vals.ptr, dB.ptr, k))
    # (not a test: eta solved again against the solution of the factor-and-solve, so that a timing of wrong results shows)
    dB.copy_from(d_eta)
    ctx.schur_sparse_solve_device(d_vals.ptr, dB.ptr, 1)
    out["solve_vs_factor_solve"] = float(np.linalg.norm(dB.download()[:n] - x) / np.linalg.norm(x))
    dB.free()
    dim = np.asarray(st.dim)
    cams = np.flatnonzero(dim == dim.max())
    sel = cams[np.linspace(0, cams.size - 1, 20).astype(np.int64)]
    out["marginals_ms"] = run(lambda: ctx.schur_sparse_marginals(d_vals.ptr, sel))
    d_sigma = api.DeviceArray(ctx, nvals)
    out["sigma_ms"] = run(lambda: ctx.schur_sparse_sigma_device(d_vals.ptr, d_sigma.ptr))
    out["sigma_inverse_ms"] = run(lambda: ctx._check(ctx.lib.spp_schur_sparse_sigma_inverse_device(ctx.h)))
    assert ctx.info("SCHUR_SPARSE_FACTOR_KEPT") == 1
    sigma = d_sigma.download()
    col_ptr, blk_off = np.asarray(st.col_ptr), np.asarray(st.blk_off)
    lms = np.flatnonzero(dim == dim.min())
    worst = 0.0
    for v in (cams[0], cams[-1], lms[0], lms[-1]):
        d = int(dim[v])
        p = int(col_ptr[v + 1]) - 1
        blk = sigma[blk_off[p]:blk_off[p] + d * d].reshape((d, d), order="F")
        cov = ctx.schur_sparse_marginals(d_vals.ptr, [int(v)])
        worst = max(worst, float(np.linalg.norm(blk - cov) / np.linalg.norm(cov)))
    out["diagonal_blocks_vs_marginals"] = worst
    out["sigma_all_finite"] = bool(np.all(np.isfinite(sigma)))
    f_ms = out["factor_solve_ms"]["median"]
    out["solve_1_over_factor_solve"] = out["solve_ms"]["1"]["median"] / f_ms
    out["sigma_over_factor_solve"] = out["sigma_ms"]["median"] / f_ms
    out["columns_times_factor_solve_ms"] = n * f_ms
    for d in [d_sigma, d_vals, d_eta, d_rhs] + d_in:
        d.free()
    ctx.set_stream(None)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="ba_banded,synthetic10k")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 20, "medians of at least 20 runs"
    lines = []
    for shape in a.shapes.split(","):
        lines.append(json.dumps(measure(shape, a.reps, a.warmup)))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
