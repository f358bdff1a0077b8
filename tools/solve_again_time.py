"""Time the solves on the kept Schur factor against the solve that leaves it, on the Venice-871 shape (871 cameras,
530 304 points, 2 838 740 observations), in one process.

    python tools/solve_again_time.py [--reps 20] [--warmup 3]

The resident path (nonlinear._ResidentBAPath) linearizes and assembles Lambda on the device once. Then, each a hipEvent
time (torch.cuda.Event on the stream the context is bound to; the stream is drained before the first event), median /
min / max of --reps runs after --warmup:
  factor_solve_ms        one spp_factor_solve_device (the existing call: what a further right-hand side cost before);
  solve_again_ms[k]      one spp_solve_device with k = 1, 6, 128 columns;
  marginals_20cam_ms     spp_marginals_device for 20 cameras (120 columns);
  marginals_20cam_20lm_ms  ... for 20 cameras and 20 landmarks (180 columns: two passes).
With --both-schedules the solves are timed in a child process each with SPP_TRSM_FUSED=1 / 0 (the switch is read once per
process). Prints one JSON line; DESIGN.md section 26 records the results."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from slam_plus_plus_amd import api, nonlinear, synth  # noqa: E402


def _stats(t):
    return {"median": float(np.median(t)), "min": float(np.min(t)), "max": float(np.max(t)), "runs": len(t)}


def measure(reps, warmup):
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
    n = int(ctx.info("N"))
    out = {"cameras": nc, "points": int(s["points"].shape[0]), "observations": int(obs.shape[0]), "n": n,
           "n_reduced": int(ctx.info("N_REDUCED")), "trsm_fused": int(os.environ.get("SPP_TRSM_FUSED", "1"))}
    out["launches_per_pass"] = (1 if out["trsm_fused"] else 2) * 2 * ((out["n_reduced"] + 127) // 128) + 4

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

    out["factor_solve_ms"] = run(factor)
    factor()
    assert ctx.info("FACTOR_KEPT") == 1
    rng = np.random.default_rng(871)
    out["solve_again_ms"] = {}
    for k in (1, 6, 128):
        B = rng.standard_normal((n, k))
        dB = api.DeviceArray.from_host(ctx, B.ravel(order="F"))
        out["solve_again_ms"][str(k)] = run(lambda: ctx.solve_device(path.d_vals.ptr, dB.ptr, k))
        dB.free()
    dim = np.asarray(path.st.dim)
    cams, lms = np.flatnonzero(dim == dim.max()), np.flatnonzero(dim == dim.min())
    sel_c = cams[np.linspace(0, cams.size - 1, 20).astype(np.int64)]
    sel_l = lms[np.linspace(0, lms.size - 1, 20).astype(np.int64)]
    for key, sel in (("marginals_20cam_ms", sel_c), ("marginals_20cam_20lm_ms", np.concatenate([sel_c, sel_l]))):
        v = np.ascontiguousarray(sel, dtype=np.int64)
        m = int(dim[v].sum())
        d_cov = api.DeviceArray(ctx, m * m)
        out[key] = run(lambda: ctx._check(ctx.lib.spp_marginals_device(ctx.h, path.d_vals.ptr, v.size, api._ptr(v), d_cov.ptr)))
        cov = d_cov.download().reshape(m, m)
        out[key]["columns"] = m
        out[key]["symmetric"] = bool(np.array_equal(cov, cov.T))
        out[key]["min_diagonal"] = float(np.diag(cov).min())
        d_cov.free()
    f, k1, k6, k128 = (out["factor_solve_ms"]["median"],) + tuple(out["solve_again_ms"][k]["median"] for k in ("1", "6", "128"))
    out["k6_over_factor_solve"] = k6 / f
    out["k128_over_128_k1"] = k128 / (128 * k1)
    path.ctx.set_stream(None)
    path.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--both-schedules", action="store_true")
    a = ap.parse_args()
    assert a.reps >= 20, "medians of at least 20 runs"
    if not a.both_schedules:
        print(json.dumps(measure(a.reps, a.warmup)))
        return
    res = {}
    for fused in ("1", "0"):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--warmup", str(a.warmup)],
                           env=dict(os.environ, SPP_TRSM_FUSED=fused), capture_output=True, text=True, check=True)
        res["one_launch_per_step" if fused == "1" else "two_launches_per_step"] = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
