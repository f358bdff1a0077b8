"""Time the Schur solve and the resident Levenberg-Marquardt iteration of a bundle adjustment with 7-wide Sim(3) cameras
against the same graph with 6-wide SE(3) cameras, on a Venice-871-shaped synthetic problem (871 cameras, 530 304 points,
2 838 740 observations) built once, in one process.

    python tools/sim3_time.py [--reps 20] [--warmup 3] [--iters 6]

For each width the resident path (nonlinear._ResidentSim3BAPath / _ResidentBAPath) linearizes and assembles Lambda on the
device once; then
  solve_ms        hipEvent time (torch.cuda.Event on the stream the context is bound to) around ONE spp_factor_solve_device,
                  median / min / max of --reps runs after --warmup;
  s_accum_ms, factor_ms
                  the library's own hipEvent brackets (spp_get_phase_ms with profiling on: phases "schur_gemm" =
                  s_accum_kernel + s_multi_kernel, and "factor" = the dense factor's launches), median of --reps further
                  solves after --warmup; profiling serialises the side stream, so these solves are not the ones above;
  lm_iteration_ms hipEvent time around one accepted iteration's work -- solve(alpha), save, gain denominator, apply, chi2 -- at a
                  fixed damping, median over the iterations after the first.
Prints one JSON line with both widths and the 7 / 6 ratios. DESIGN.md section 23 records the results."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from slam_plus_plus_amd import formats, nonlinear, synth  # noqa: E402


def _scene(seed=871):
    """the Venice-871 shape of synth.CONFIGS: observation lists of ba_problem, cameras of ba_states. The Sim(3) camera of an
    SE(3) camera (R, t) world -> camera is the pose (R^T, -R^T t, e^s), s uniform in [-0.3, 0.3]; each family gets the
    measurements of its own projection + 0.5 px noise, no distortion."""
    from scipy.spatial.transform import Rotation
    p = synth.make("venice871")
    s = synth.ba_states(p)
    rng = np.random.default_rng(seed)
    cams6 = s["cams"]
    nc = cams6.shape[0]
    intr = np.tile(np.array([500.0, 505.0, 320.0, 240.0, 0.0]), (nc, 1))
    co, po = s["cam_of"].astype(np.int64), s["pt_of"].astype(np.int64)
    R = Rotation.from_rotvec(cams6[:, 3:])
    trs = np.concatenate([-R.inv().apply(cams6[:, :3]), R.inv().as_rotvec(), np.exp(rng.uniform(-0.3, 0.3, size=(nc, 1)))], axis=1)
    cams7 = formats.sim3_from_trs(trs)
    pts = s["points"] + rng.normal(0, 0.01, size=s["points"].shape)
    noise = rng.normal(0, 0.5, size=(co.size, 2))
    ids = np.stack([co.astype(np.float64), po.astype(np.float64)], axis=1)
    uv7 = formats.sim3_expectation(cams7[co], intr[co], s["points"][po])[0]
    x = R[co].apply(s["points"][po]) + cams6[co, :3]
    uv6 = intr[co, 2:4] + intr[co, :2] * x[:, :2] / x[:, 2:3]
    return (cams6, np.concatenate([ids, uv6 + noise], axis=1)), (cams7, np.concatenate([ids, uv7 + noise], axis=1)), intr, pts


def _stats(t):
    return {"median": float(np.median(t)), "min": float(np.min(t)), "max": float(np.max(t)), "runs": len(t)}


def _measure(path, system, reps, warmup, iters):
    import torch
    stream = torch.cuda.Stream()
    path.ctx.set_stream(stream.cuda_stream)

    def timed(f):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        f()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    path.begin(system)
    path.linearize()
    alpha = 1e-3 * path.max_hessian_diag()
    path.chi2()
    path._assemble(alpha)
    path._analyze_once()
    ctx = path.ctx
    out = {"mode": int(ctx.info("MODE")), "n_reduced": int(ctx.info("N_REDUCED"))}

    def solve():
        path.d_dx.copy_from(path.d_eta)
        stream.synchronize()
        t = timed(lambda: ctx.factor_solve_device(path.d_vals.ptr, path.d_dx.ptr))
        return t

    t = [solve() for _ in range(warmup + reps)][warmup:]
    out["solve_ms"] = _stats(t)
    ctx.set_profiling(True)
    ph = []
    for _ in range(warmup + reps):
        solve()
        ph.append(ctx.phase_ms())
    ctx.set_profiling(False)
    ph = ph[warmup:]
    out["s_accum_ms"] = _stats([q["schur_gemm"] for q in ph])
    out["factor_ms"] = _stats([q["factor"] for q in ph])

    def iteration():
        ok, _ = path.solve(alpha)
        assert ok
        path.save()
        path.gain_denominator(alpha)
        path.apply()
        path.chi2()

    t = [timed(iteration) for _ in range(iters)]
    out["lm_first_iteration_ms"], out["lm_iteration_ms"] = t[0], _stats(t[1:])
    path.ctx.set_stream(None)
    path.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=6)
    a = ap.parse_args()
    assert a.reps >= 20, "medians of at least 20 runs"
    import torch
    torch.cuda.init()   # before the library opens the device (as bench.py and tools/stereo_time.py do)
    (cams6, obs6), (cams7, obs7), intr, pts = _scene()
    out = {"cameras": int(cams6.shape[0]), "points": int(pts.shape[0]), "observations": int(obs6.shape[0])}
    out["se3_6"] = _measure(nonlinear._ResidentBAPath(), nonlinear.CBundleAdjustment(cams6, intr, pts, obs6), a.reps, a.warmup, a.iters)
    out["sim3_7"] = _measure(nonlinear._ResidentSim3BAPath(), nonlinear.CBundleAdjustmentSim3(cams7, intr, pts, obs7), a.reps, a.warmup, a.iters)
    for k in ("solve_ms", "s_accum_ms", "factor_ms", "lm_iteration_ms"):
        out["ratio_7_over_6_" + k] = out["sim3_7"][k]["median"] / out["se3_6"][k]["median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
