"""Time the stereo projection kernel and the resident Levenberg-Marquardt iteration of a stereo bundle adjustment on a
Venice-871-shaped synthetic problem (871 cameras, 530 304 points, 2 838 740 observations), the mono figures of the same
geometry beside them.

    python tools/stereo_time.py [--reps 20] [--warmup 3] [--iters 6]

Kernel figures: hipEvent time (torch.cuda.Event on the stream the context is bound to) around --reps back-to-back
launches of spp_ba_stereo_linearize_device / spp_ba_linearize_device, divided by --reps, after --warmup launches; the
same cameras, points and observation lists for both (the mono kernel reads the first 5 intrinsics and u v).
LM figures: wall time of one accepted iteration's device work -- solve(alpha), save, gain denominator, apply, chi2 -- of
nonlinear._ResidentStereoBAPath / _ResidentBAPath with a fixed damping, median over the iterations after the first
(which holds the symbolic analysis). Prints one JSON line. DESIGN.md section 16 records the results."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from slam_plus_plus_amd import api, formats, nonlinear, synth  # noqa: E402


def _scene(seed=871):
    """the Venice-871 shape of synth.CONFIGS with stereo cameras: observation lists of ba_problem, cameras of ba_states,
    six intrinsics (d = 0.1 on every odd camera, baseline 0.5), measurements = the stereo expectation + 0.5 px noise"""
    p = synth.make("venice871")
    s = synth.ba_states(p)
    rng = np.random.default_rng(seed)
    nc = s["cams"].shape[0]
    intr = np.tile(np.array([500.0, 505.0, 320.0, 240.0, 0.0, 0.5]), (nc, 1))
    intr[1::2, 4] = 0.1
    co, po = s["cam_of"].astype(np.int64), s["pt_of"].astype(np.int64)
    pts = s["points"] + rng.normal(0, 0.01, size=s["points"].shape)
    meas = formats.stereo_expectation(s["cams"][co], intr[co], s["points"][po]) + rng.normal(0, 0.5, size=(co.size, 3))
    obs = np.concatenate([co[:, None].astype(np.float64), po[:, None].astype(np.float64), meas], axis=1)
    return s["cams"], intr, pts, obs


def _kernel_ms(ctx, call, reps, warmup):
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


def _lm_ms(path, system, iters):
    path.begin(system)
    path.linearize()
    alpha = 1e-3 * path.max_hessian_diag()
    path.chi2()
    t = []
    for _ in range(iters):
        t0 = time.perf_counter()
        ok, _ = path.solve(alpha)
        path.save()
        path.gain_denominator(alpha)
        path.apply()
        path.chi2()
        t.append(1e3 * (time.perf_counter() - t0))
        assert ok
    path.close()
    return t[0], float(np.median(t[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=6)
    a = ap.parse_args()
    import torch
    torch.cuda.init()   # before the library opens the device (as bench.py and tools/dense_time.py --vendor do)
    cams, intr, pts, obs = _scene()
    no = obs.shape[0]
    out = {"cameras": int(cams.shape[0]), "points": int(pts.shape[0]), "observations": int(no)}
    ctx = api.Context(0)
    up = lambda x: api.DeviceArray.from_host(ctx, np.ascontiguousarray(x).ravel())
    d_co, d_po = up(obs[:, 0].astype(np.int32)), up(obs[:, 1].astype(np.int32))
    d_c, d_p = up(cams), up(pts)
    # the mono kernel is fed the stereo lens as it is: under Project_P2C's rho^2 law d = 0.1 is a far stronger distortion,
    # which changes the values it computes and not the work it does; the LM part below, whose path must converge, zeroes it
    for key, entry, rd, d_i, d_m in (("stereo", ctx.ba_stereo_linearize_device, 3, up(intr), up(obs[:, 2:5])),
                                     ("mono", ctx.ba_linearize_device, 2, up(intr[:, :5]), up(obs[:, 2:4]))):
        J0, J1, r = api.DeviceArray(ctx, 6 * rd * no), api.DeviceArray(ctx, 3 * rd * no), api.DeviceArray(ctx, rd * no)
        ms = _kernel_ms(ctx, lambda: entry(no, d_co.ptr, d_po.ptr, d_c.ptr, d_i.ptr, d_p.ptr, d_m.ptr, J0.ptr, J1.ptr, r.ptr),
                        a.reps, a.warmup)
        moved = no * (4 * 2 + 8 * (6 + (6 if rd == 3 else 5) + 3 + rd) + 8 * 10 * rd)   # gathers counted once per observation
        out[key + "_linearize_ms"], out[key + "_linearize_gb_per_s"] = ms, moved / ms * 1e-6
        for d in (J0, J1, r, d_i, d_m):
            d.free()
    ctx.close()
    s = nonlinear.CStereoBundleAdjustment(cams, intr, pts, obs)
    out["stereo_lm_first_iteration_ms"], out["stereo_lm_iteration_ms"] = _lm_ms(nonlinear._ResidentStereoBAPath(), s, a.iters)
    intr5 = intr[:, :5].copy()
    intr5[:, 4] = 0.0   # Project_P2C's distortion is quadratic in rho: the stereo d would be another lens
    m = nonlinear.CBundleAdjustment(cams, intr5, pts, obs[:, :4])
    out["mono_lm_first_iteration_ms"], out["mono_lm_iteration_ms"] = _lm_ms(nonlinear._ResidentBAPath(), m, a.iters)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
