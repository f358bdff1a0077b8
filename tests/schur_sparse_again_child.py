"""Child process of tests/test_gpu_schur_sparse_again.py: the library reads its switches once per process, so every variant
is one run of this file with the switches in its environment.

    python schur_sparse_again_child.py INPUT.npz OUTPUT.npz SYSTEM[,SYSTEM...]

Every named system of INPUT (written by the parent from tests/schur_sparse_again_ref.py) is analyzed in MODE_SCHUR_SPARSE.
Per system:
  base_B     the existing path on every column of B and on the unit columns of the marginal vertices: one
             spp_factor_solve_device each, in this mode
  X1, X6 ..  spp_schur_sparse_solve_device on NaN-framed copies (ldb = n + 3, a spare column) of the leading 1, 6, 17 (129)
             columns of B; `again`: all of them once more at ldb = n; alone<j>: column j by itself
  marg       schur_sparse_marginals of the marginal vertices, jointly
  sigma      spp_schur_sparse_sigma_device into a NaN-filled buffer between NaN guards; sigma2 a second call; X_before /
             X_after: a two-column solve on either side of the first
  base       in the layout of vals, the existing path of the covariance blocks: spp_solve_device on the unit columns of the
             checked vertices in a second ctx analyzed in MODE_SCHUR (dense reduced system), read at the rows of the
             column's stored blocks (NaN elsewhere)
  route      (`full` systems) the same blocks from spp_schur_sparse_solve_device on all n unit columns
and beside them spp_factor_solve_device(eta) before, after and on a ctx that never made the new calls, the three info
words, the front table, schur_sparse_sigma(), schur_sparse_block_diagonal(). This process asserts the return codes of the
healthy calls only; everything else is the parent's."""
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
ALONE = (0, 15, 16, 127, 128)   # the column positions of tests/sparse_solve_child.py
FRONT_KEYS = ("h", "w", "pad", "cls", "level", "parent", "team")
WORDS = ("SCHUR_SPARSE_FACTOR_KEPT", "FACTOR_KEPT", "SPARSE_FACTOR_KEPT")


def system(inp, name):
    g = lambda k: inp["%s/%s" % (name, k)]  # noqa: E731
    return BlockCSC(g("dim"), g("col_ptr"), g("row_idx"), g("blk_off"), g("vals")), g("eta"), g("B")


def words(c):
    return [c.info(w) for w in WORDS]


def factor(c, dv, eta):
    dr = api.DeviceArray.from_host(c, eta)
    st = c.factor_solve_device(dv.ptr, dr.ptr)
    x = dr.download()
    dr.free()
    return st, x


def baseline(c, dv, B):
    out = np.empty_like(B)
    for j in range(B.shape[1]):
        st, out[:, j] = factor(c, dv, np.ascontiguousarray(B[:, j]))
        assert st == 0
    return out


def framed_solve(c, dv, B, ldb=None, extra_cols=1):
    """spp_schur_sparse_solve_device on a NaN-framed copy of B: (the n x k result, whether the frame is untouched)"""
    n, k = B.shape
    ldb = n + 3 if ldb is None else ldb
    buf = np.full((ldb, k + extra_cols), np.nan, order="F")
    buf[:n, :k] = B
    dB = api.DeviceArray.from_host(c, buf.ravel(order="F"))
    assert c.schur_sparse_solve_device(dv.ptr, dB.ptr, k, ldb) == 0
    out = dB.download().reshape((ldb, k + extra_cols), order="F")   # (the download is ordered behind the solve)
    dB.free()
    return out[:n, :k].copy(), bool(np.all(np.isnan(out[n:, :])) and np.all(np.isnan(out[:, k:])))


def framed_sigma(c, dv, nvals):
    """spp_schur_sparse_sigma_device into the middle of a NaN-filled buffer: (sigma, whether both guards are untouched)"""
    d = api.DeviceArray.from_host(c, np.full(nvals + 2 * GUARD, np.nan))
    assert c.schur_sparse_sigma_device(dv.ptr, d.ptr + 8 * GUARD) == 0
    out = d.download()
    d.free()
    return out[GUARD:GUARD + nvals].copy(), bool(np.all(np.isnan(out[:GUARD])) and np.all(np.isnan(out[GUARD + nvals:])))


def solve_route(solve, lam, index, vertices):
    """Sigma on the pattern from solve(E) on the unit columns of `vertices`, in passes of 128"""
    pos, r, col, _ = index
    out = np.full(lam.nvals, np.nan)
    n = lam.n
    cols = np.concatenate([np.arange(lam.base[v], lam.base[v + 1]) for v in vertices])
    for k0 in range(0, cols.size, PASS):
        sel = cols[k0:k0 + PASS]
        E = np.zeros((n, sel.size), order="F")
        E[sel, np.arange(sel.size)] = 1.0
        X = solve(E)
        at = np.full(n, -1, dtype=np.int64)
        at[sel] = np.arange(sel.size)
        m = at[col] >= 0
        out[pos[m]] = X[r[m], at[col[m]]]
    return out


def dense_solve(c, dv, B):
    n, k = B.shape
    d = api.DeviceArray.from_host(c, np.asfortranarray(B).ravel(order="F"))
    assert c.solve_device(dv.ptr, d.ptr, k, n) == 0
    X = d.download().reshape((n, k), order="F")
    d.free()
    return X


def one_system(inp, out, name, full):
    lam, eta, B = system(inp, name)
    check = inp[name + "/check"]
    sel = inp[name + "/sel"]
    index = sgr.pattern_index(lam)
    c = api.Context(0)
    c.analyze(lam, api.MODE_SCHUR_SPARSE)
    assert c.info("MODE") == api.MODE_SCHUR_SPARSE
    fr = c.sparse_fronts()
    for k in FRONT_KEYS:
        out["%s/front_%s" % (name, k)] = fr[k]
    dv = api.DeviceArray.from_host(c, lam.vals)
    kept = [words(c)]
    out[name + "/base_B"] = baseline(c, dv, B)
    E_sel = np.zeros((lam.n, int(lam.dim[sel].sum())))
    rows = np.concatenate([np.arange(lam.base[v], lam.base[v + 1]) for v in sel])
    E_sel[rows, np.arange(rows.size)] = 1.0
    out[name + "/base_marg"] = baseline(c, dv, E_sel)[rows]
    st, x_eta = factor(c, dv, eta)
    assert st == 0
    out[name + "/x_eta"] = x_eta
    kept.append(words(c))
    frames = []
    kmax = B.shape[1]
    for k in (1, 6, 17) + ((kmax,) if kmax > 17 else ()):
        out["%s/X%d" % (name, k)], ok = framed_solve(c, dv, B[:, :k])
        frames.append(ok)
    out[name + "/again"], ok = framed_solve(c, dv, B, ldb=lam.n, extra_cols=2)
    frames.append(ok)
    for j in ALONE:
        if j < kmax:
            out["%s/alone%d" % (name, j)], ok = framed_solve(c, dv, B[:, j:j + 1])
            frames.append(ok)
    out[name + "/marg"] = c.schur_sparse_marginals(dv.ptr, sel)
    kept.append(words(c))
    B2 = np.stack([eta, np.arange(1.0, lam.n + 1.0)], axis=1)
    out[name + "/X_before"], ok = framed_solve(c, dv, B2)
    frames.append(ok)
    out[name + "/sigma"], ok = framed_sigma(c, dv, lam.nvals)
    frames.append(ok)
    kept.append(words(c))
    out[name + "/X_after"], ok = framed_solve(c, dv, B2)
    frames.append(ok)
    out[name + "/sigma2"], ok = framed_sigma(c, dv, lam.nvals)
    frames.append(ok)
    out[name + "/frames"] = np.array(frames)
    out[name + "/sigma_host"] = c.schur_sparse_sigma(dv.ptr)
    diag = c.schur_sparse_block_diagonal(dv.ptr)
    out[name + "/n_diag"] = np.int64(len(diag))
    out[name + "/diag_all"] = np.concatenate([D.ravel(order="F") for D in diag])   # every vertex's block, in vertex order
    if full:
        out[name + "/route"] = solve_route(lambda E: framed_solve(c, dv, E, ldb=lam.n, extra_cols=0)[0], lam, index,
                                           np.arange(lam.nb))
    kept.append(words(c))
    st, out[name + "/x_eta_after"] = factor(c, dv, eta)
    assert st == 0
    kept.append(words(c))
    out[name + "/kept"] = np.array(kept)
    dv.free()
    c.close()
    # a ctx that never made the new calls: spp_factor_solve_device gives the same bits
    c = api.Context(0)
    c.analyze(lam, api.MODE_SCHUR_SPARSE)
    dv = api.DeviceArray.from_host(c, lam.vals)
    st, out[name + "/x_eta_fresh"] = factor(c, dv, eta)
    assert st == 0
    dv.free()
    c.close()
    # the existing path of the covariance blocks: the dense reduced system
    c = api.Context(0)
    c.analyze(lam, api.MODE_SCHUR)
    dv = api.DeviceArray.from_host(c, lam.vals)
    assert factor(c, dv, eta)[0] == 0
    out[name + "/base"] = solve_route(lambda E: dense_solve(c, dv, E), lam, index, check)
    dv.free()
    c.close()


def main():
    inp = np.load(sys.argv[1])
    out = {"env": np.array(sorted("%s=%s" % kv for kv in os.environ.items() if kv[0].startswith("SPP_") and kv[0] != "SPP_LIB"))}
    full = set(inp["full"].tolist())
    for name in sys.argv[3].split(","):
        one_system(inp, out, name, name in full)
    np.savez(sys.argv[2], **out)
    print("ok: %d arrays" % len(out))


if __name__ == "__main__":
    main()
