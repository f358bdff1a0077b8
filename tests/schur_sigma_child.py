"""Child process of tests/test_gpu_schur_sigma.py: the library reads its switches once per process, so every variant is
one run of this file with the switches in its environment.

    python schur_sigma_child.py INPUT.npz OUTPUT.npz SYSTEM[,SYSTEM...]

Every named system of INPUT (written by the parent from tests/schur_sigma_ref.py) is analyzed in MODE_SCHUR. Per system,
in the layout of vals:
  base     the existing path on the unit columns of the checked vertices -- spp_solve_device in passes of 128 --, read at
           the rows of the column's stored blocks (NaN elsewhere)
  sigma    spp_schur_sigma_device into a NaN-filled buffer between NaN guards; sigma2 a second call
and beside them the solves before and after the call, spp_factor_solve_device(eta) after it and on a ctx that never made
it, the flags, schur_sigma(), every block of schur_block_diagonal() and marginals([v]) of the selected vertices. This process asserts
the return codes of the healthy calls only; everything else is the parent's."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from slam_plus_plus_amd import api  # noqa: E402
import sparse_sigma_ref as sgr  # noqa: E402
from slam_plus_plus_amd.blockcsc import BlockCSC  # noqa: E402

GUARD = 8       # NaN doubles in front of and behind d_sigma
PASS = 128


def system(inp, name):
    g = lambda k: inp["%s/%s" % (name, k)]  # noqa: E731
    return BlockCSC(g("dim"), g("col_ptr"), g("row_idx"), g("blk_off"), g("vals")), g("eta")


def factor(c, dv, eta):
    dr = api.DeviceArray.from_host(c, eta)
    st = c.factor_solve_device(dv.ptr, dr.ptr)
    x = dr.download()
    dr.free()
    return st, x


def solve(c, dv, B):
    n, k = B.shape
    d = api.DeviceArray.from_host(c, np.asfortranarray(B).ravel(order="F"))
    assert c.solve_device(dv.ptr, d.ptr, k, n) == 0
    X = d.download().reshape((n, k), order="F")
    d.free()
    return X


def framed_sigma(c, dv, nvals):
    """spp_schur_sigma_device into the middle of a NaN-filled buffer: (sigma, whether both guards are untouched)"""
    d = api.DeviceArray.from_host(c, np.full(nvals + 2 * GUARD, np.nan))
    assert c.schur_sigma_device(dv.ptr, d.ptr + 8 * GUARD) == 0
    out = d.download()
    d.free()
    return out[GUARD:GUARD + nvals].copy(), bool(np.all(np.isnan(out[:GUARD])) and np.all(np.isnan(out[GUARD + nvals:])))


def solve_route(c, dv, lam, index, vertices):
    """Sigma on the pattern from spp_solve_device on the unit columns of `vertices`, in passes of 128"""
    pos, r, col, _ = index
    out = np.full(lam.nvals, np.nan)
    n = lam.n
    cols = np.concatenate([np.arange(lam.base[v], lam.base[v + 1]) for v in vertices])
    for k0 in range(0, cols.size, PASS):
        sel = cols[k0:k0 + PASS]
        E = np.zeros((n, sel.size), order="F")
        E[sel, np.arange(sel.size)] = 1.0
        X = solve(c, dv, E)
        at = np.full(n, -1, dtype=np.int64)
        at[sel] = np.arange(sel.size)
        m = at[col] >= 0
        out[pos[m]] = X[r[m], at[col[m]]]
    return out


def one_system(inp, out, name):
    lam, eta = system(inp, name)
    check = inp[name + "/check"]
    sel = inp[name + "/sel"]
    index = sgr.pattern_index(lam)
    c = api.Context(0)
    c.analyze(lam, api.MODE_SCHUR)
    dv = api.DeviceArray.from_host(c, lam.vals)
    st, x_eta = factor(c, dv, eta)
    assert st == 0
    out[name + "/x_eta"] = x_eta
    kept = [c.info("FACTOR_KEPT")]
    out[name + "/base"] = solve_route(c, dv, lam, index, check)
    B = np.stack([eta, np.arange(1.0, lam.n + 1.0)], axis=1)
    out[name + "/X_before"] = solve(c, dv, B)
    frames = []
    out[name + "/sigma"], ok = framed_sigma(c, dv, lam.nvals)
    frames.append(ok)
    kept.append(c.info("FACTOR_KEPT"))
    out[name + "/X_after"] = solve(c, dv, B)
    out[name + "/sigma2"], ok = framed_sigma(c, dv, lam.nvals)
    frames.append(ok)
    out[name + "/frames"] = np.array(frames)
    out[name + "/sigma_host"] = c.schur_sigma(dv.ptr)
    diag = c.schur_block_diagonal(dv.ptr)
    out[name + "/n_diag"] = np.int64(len(diag))
    out[name + "/diag_all"] = np.concatenate([D.ravel(order="F") for D in diag])   # every vertex's block, in vertex order
    for v in sel:
        out["%s/diag%d" % (name, v)] = diag[int(v)]
        out["%s/marg%d" % (name, v)] = c.marginals(dv.ptr, [int(v)])
    kept.append(c.info("FACTOR_KEPT"))
    st, out[name + "/x_eta_after"] = factor(c, dv, eta)
    assert st == 0
    out[name + "/kept"] = np.array(kept)
    dv.free()
    c.close()
    # a ctx that never made the call: spp_factor_solve_device gives the same bits
    c = api.Context(0)
    c.analyze(lam, api.MODE_SCHUR)
    dv = api.DeviceArray.from_host(c, lam.vals)
    st, out[name + "/x_eta_fresh"] = factor(c, dv, eta)
    assert st == 0
    dv.free()
    c.close()


def main():
    inp = np.load(sys.argv[1])
    out = {"env": np.array(sorted("%s=%s" % kv for kv in os.environ.items() if kv[0].startswith("SPP_") and kv[0] != "SPP_LIB"))}
    for name in sys.argv[3].split(","):
        one_system(inp, out, name)
    np.savez(sys.argv[2], **out)
    print("ok: %d arrays" % len(out))


if __name__ == "__main__":
    main()
