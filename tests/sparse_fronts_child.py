"""Child process of tests/test_gpu_sparse_fronts.py: the library reads its switches once per process, so every variant
is one run of this file with the switches in its environment.

    python sparse_fronts_child.py INPUT.npz OUTPUT.npz designed FIXTURE[,FIXTURE...] [fail]
    python sparse_fronts_child.py INPUT.npz OUTPUT.npz pose

designed: every named system of INPUT (written by the parent from tests/sparse_fixtures.py) is solved with
CLinearSolver_HIP(mode=MODE_SPARSE) four times on one solver object -- twice, then with another right-hand side, then the
first again -- and x of each solve, the front table and the ordering go to OUTPUT. `fail`: the failure paths of INPUT's
`fail_*` entries as well. pose: se2_small and se3_small assembled with damping=50.
This process asserts the return codes only; everything else is the parent's."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from slam_plus_plus_amd import api  # noqa: E402
from slam_plus_plus_amd.blockcsc import BlockCSC  # noqa: E402

FRONT_KEYS = ("h", "w", "pad", "cls", "level", "parent", "team")


def table(solver, out, name, nb):
    fr = solver.ctx.sparse_fronts()
    assert fr["h"].size == solver.ctx.info("N_SUPERNODES") > 0
    for k in FRONT_KEYS:
        out["%s/front_%s" % (name, k)] = fr[k]
    out[name + "/order"] = solver.ctx.ordering(nb)
    out[name + "/levels"] = np.int64(solver.ctx.info("N_LEVELS"))


def solve(solver, lam, rhs):
    x = rhs.copy()
    assert solver.Solve_PosDef_Blocky(lam, x), "factorization failed"
    return x


def broken(solver, lam, eta, offset, value, out, tag):
    """one value of Lambda replaced: the designed error return, then the healthy system on the same solver object"""
    vals = lam.vals.copy()
    vals[offset] = value
    x = eta.copy()
    assert solver.Solve_PosDef_Blocky(lam.with_vals(vals), x) is False, "a broken pivot was not reported"
    out[tag + "/rhs_after"] = x
    out[tag + "/x_after"] = solve(solver, lam, eta)


def designed(inp, out, names, fail):
    for name in names:
        g = lambda k: inp["%s/%s" % (name, k)]  # noqa: E731
        lam = BlockCSC(g("dim"), g("col_ptr"), g("row_idx"), g("blk_off"), g("vals"))
        eta, eta2 = g("eta"), g("eta2")
        solver = api.CLinearSolver_HIP(mode=api.MODE_SPARSE)
        out[name + "/x1"] = solve(solver, lam, eta)
        out[name + "/x2"] = solve(solver, lam, eta)       # the next epoch and solve_index
        out[name + "/y"] = solve(solver, lam, eta2)
        out[name + "/x3"] = solve(solver, lam, eta)
        table(solver, out, name, lam.nb)
        if fail:
            tags = [str(t) for t in inp["fail_tags"] if str(t).split(":")[0] == name]
            for tag in tags:
                offset, value = inp["fail_offset/" + tag], inp["fail_value/" + tag]
                broken(solver, lam, eta, int(offset), float(value), out, "fail/" + tag)


def pose(out):
    from slam_plus_plus_amd import synth
    from oracle import spp_oracle as orc
    for name in ("se2_small", "se3_small"):
        lam, eta = orc.assemble(synth.make(name), damping=50.0)
        solver = api.CLinearSolver_HIP(mode=api.MODE_SPARSE)
        out[name + "/x1"] = solve(solver, lam, eta)
        out[name + "/x2"] = solve(solver, lam, eta)
        table(solver, out, name, lam.nb)


def main():
    inp = np.load(sys.argv[1])
    out = {}
    if sys.argv[3] == "pose":
        pose(out)
    else:
        designed(inp, out, sys.argv[4].split(","), "fail" in sys.argv[5:])
    np.savez(sys.argv[2], **out)
    print("ok: %d arrays" % len(out))


if __name__ == "__main__":
    main()
