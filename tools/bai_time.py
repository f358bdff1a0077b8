"""Time the assembly of ternary edges and the resident Levenberg-Marquardt iteration of a bundle adjustment with ONE shared
intrinsics vertex on a Venice-871-shaped synthetic problem (871 cameras, 530 304 points, 2 838 740 observations), the
mono figures of the same cameras, points and observations beside them, in the same run.

    python tools/bai_time.py [--reps 20] [--warmup 3] [--iters 6]

Assembly figures: hipEvent time (torch.cuda.Event on the stream the context is bound to) around --reps back-to-back calls
of spp_assemble_ternary_device / spp_assemble_device, divided by --reps, after --warmup calls. The ternary call runs the
mono kernels on the (camera, point) part and the border kernels on top: H02 per camera (871 destinations of about 3 260
edges), one H12 per point, H22 and g2 of the hub (2 838 740 edges: 694 chunks). LM figures: one accepted
iteration's work -- solve(alpha), save, gain denominator, apply, chi2 -- of nonlinear._ResidentBAIPath / _ResidentBAPath
with a fixed damping, measured twice: *_lm_iteration_event_ms is the hipEvent time around --iters - 1 iterations back to
back on the context's stream, divided by their number (the stream is synchronized inside an iteration wherever a scalar goes
to the host, so the figure holds those waits), after the first iteration, which holds the symbolic analysis;
*_lm_iteration_ms is the host's wall clock per iteration (time.perf_counter, median). Prints one JSON line. DESIGN.md section 20 records the results."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from slam_plus_plus_amd import api, formats, nonlinear, synth  # noqa: E402


def _scene(seed=871):
    """the Venice-871 shape of synth.CONFIGS: observation lists of ba_problem, cameras and points of ba_states, one
    intrinsics vertex (fx 500, fy 505, kappa = 2 % at 200 px), measurements = the expectation + 0.5 px noise"""
    p = synth.make("venice871")
    s = synth.ba_states(p)
    rng = np.random.default_rng(seed)
    intr = np.array([[500.0, 505.0, 320.0, 240.0, 0.02 * 502.5 / 200.0 ** 2]])
    co, po = s["cam_of"].astype(np.int64), s["pt_of"].astype(np.int64)
    io = np.zeros(co.size, dtype=np.int64)
    pts = s["points"] + rng.normal(0, 0.01, size=s["points"].shape)
    meas = formats.bai_expectation(s["cams"][co], intr[io], s["points"][po]) + rng.normal(0, 0.5, size=(co.size, 2))
    f = lambda a: a[:, None].astype(np.float64)
    return s["cams"], intr, pts, np.concatenate([f(co), f(po), f(io), meas], axis=1)


def _event_ms(ctx, call, reps, warmup):
    import torch
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    for _ in range(warmup):
        call()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(reps):
        call()
    b.record(stream)
    b.synchronize()
    ctx.set_stream(None)
    return a.elapsed_time(b) / reps


def _lm_ms(path, system, iters, hook=None):
    path.begin(system)
    path.linearize()
    alpha = 1e-3 * path.max_hessian_diag()
    path.chi2()
    extra = hook(path, alpha) if hook else {}
    t = []

    def iteration():
        t0 = time.perf_counter()
        ok, _ = path.solve(alpha)
        path.save()
        path.gain_denominator(alpha)
        path.apply()
        path.chi2()
        t.append(1e3 * (time.perf_counter() - t0))
        assert ok

    iteration()     # holds the symbolic analysis
    extra["event_ms"] = _event_ms(path.ctx, iteration, iters - 1, 0)
    path.close()
    return t[0], float(np.median(t[1:])), extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=6)
    a = ap.parse_args()
    import torch
    torch.cuda.init()   # before the library opens the device (as bench.py does)
    cams, intr, pts, obs = _scene()
    out = {"cameras": int(cams.shape[0]), "points": int(pts.shape[0]), "observations": int(obs.shape[0]), "intrinsics": 1}

    def ternary(p, alpha):
        ms = _event_ms(p.ctx, lambda: p.ctx.assemble_ternary_device(p.d_J0.ptr, p.d_J1.ptr, p.d_J2.ptr, p.d_Om.ptr, p.d_r.ptr,
                                                                     alpha, p.d_vals.ptr, p.d_eta.ptr), a.reps, a.warmup)
        return {"assemble_ternary_ms": ms, "hub_chunk": p.ctx.info("ASM_HUB_CHUNK")}

    def mono(p, alpha):
        ms = _event_ms(p.ctx, lambda: p.ctx.assemble_device(p.d_J0.ptr, p.d_J1.ptr, p.d_Om.ptr, p.d_r.ptr, alpha, p.d_vals.ptr,
                                                             p.d_eta.ptr), a.reps, a.warmup)
        return {"assemble_mono_ms": ms}

    s = nonlinear.CBundleAdjustmentIntrinsics(cams, intr, pts, obs)
    t0 = time.perf_counter()
    out["bai_lm_first_iteration_ms"], out["bai_lm_iteration_ms"], e = _lm_ms(nonlinear._ResidentBAIPath(), s, a.iters, ternary)
    out["bai_lm_iteration_event_ms"] = e.pop("event_ms")
    out.update(e)
    out["bai_total_s"] = time.perf_counter() - t0
    m = nonlinear.CBundleAdjustment(cams, np.tile(intr, (cams.shape[0], 1)), pts, obs[:, [0, 1, 3, 4]])
    out["mono_lm_first_iteration_ms"], out["mono_lm_iteration_ms"], e = _lm_ms(nonlinear._ResidentBAPath(), m, a.iters, mono)
    out["mono_lm_iteration_event_ms"] = e.pop("event_ms")
    out.update(e)
    out["border_ms"] = out["assemble_ternary_ms"] - out["assemble_mono_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
