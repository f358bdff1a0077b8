"""Time the solves on the kept SPARSE factor against the solve that leaves it, on the two pose-graph shapes
(sphere2500, manhattan3500), in one process.

    python tools/sparse_solve_again_time.py [--reps 20] [--warmup 3] [--shape SHAPE] [--out profiles/NAME.json]

Per shape Lambda is assembled on the device as bench.py assembles it and analyzed in SPP_MODE_SPARSE. Then, each a
hipEvent time (torch.cuda.Event on the stream the context is bound to; the stream is drained before the first event),
median / min / max of --reps runs after --warmup:
  factor_solve_ms        one spp_factor_solve_device (the existing call: what a further right-hand side cost before);
  solve_again_ms[k]      one spp_sparse_solve_device with k = 1, 6, 128 columns;
  marginals_20_ms        spp_sparse_marginals_device for 20 poses spread over the trajectory;
  launches_per_pass      kernel launches of one pass of at most 128 columns (from the front table).
The expectation DESIGN.md section 27 states is k6_over_factor_solve < 1 on both shapes. Prints one JSON line and, with
--out, writes it to that file."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from slam_plus_plus_amd import api, synth  # noqa: E402

SHAPES = ("sphere2500", "manhattan3500")


def _stats(t):
    return {"median": float(np.median(t)), "min": float(np.min(t)), "max": float(np.max(t)), "runs": len(t)}


def launches_per_pass(fr):
    """gather, per level and direction one launch for the fronts of classes 0 - 2 and one for those of classes 3 - 4, scatter"""
    groups = set((int(l), int(c) >= 3) for l, c in zip(fr["level"], fr["cls"]))
    return 2 * len(groups) + 2


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
    out = {"poses": int(st.nb), "n": n, "supernodes": int(ctx.info("N_SUPERNODES")), "levels": int(ctx.info("N_LEVELS")),
           "launches_per_pass": launches_per_pass(ctx.sparse_fronts())}

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
    x = d_rhs.download()
    rng = np.random.default_rng(2500)
    out["solve_again_ms"] = {}
    for k in (1, 6, 128):
        B = rng.standard_normal((n, k))
        B[:, 0] = d_eta.download()
        dB = api.DeviceArray.from_host(ctx, B.ravel(order="F"))
        ctx.sparse_solve_device(dB.ptr, k)
        X0 = dB.download()[:n]
        # (not a test: the column of eta against the solve that left the factor, so that a timing of wrong results shows)
        out.setdefault("eta_column_vs_factor_solve", {})[str(k)] = float(np.linalg.norm(X0 - x) / np.linalg.norm(x))
        dB.upload(B.ravel(order="F"))
        out["solve_again_ms"][str(k)] = run(lambda: ctx.sparse_solve_device(dB.ptr, k))
        dB.free()
    dim = np.asarray(st.dim)
    v = np.ascontiguousarray(np.linspace(0, st.nb - 1, 20).astype(np.int64))
    m = int(dim[v].sum())
    d_cov = api.DeviceArray(ctx, m * m)
    out["marginals_20_ms"] = run(lambda: ctx._check(ctx.lib.spp_sparse_marginals_device(ctx.h, v.size, api._ptr(v), d_cov.ptr)))
    cov = d_cov.download().reshape(m, m)
    out["marginals_20_ms"].update(columns=m, symmetric=bool(np.array_equal(cov, cov.T)), min_diagonal=float(np.diag(cov).min()))
    d_cov.free()
    f, k1, k6, k128 = (out["factor_solve_ms"]["median"],) + tuple(out["solve_again_ms"][k]["median"] for k in ("1", "6", "128"))
    out["k6_over_factor_solve"] = k6 / f
    out["k128_over_128_k1"] = k128 / (128 * k1)
    for d in d_in + [d_vals, d_eta, d_rhs]:
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
