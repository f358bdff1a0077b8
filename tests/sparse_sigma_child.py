"""Child process of tests/test_gpu_sparse_sigma.py: the library reads its switches once per process, so every variant is
one run of this file with the switches in its environment.

    python sparse_sigma_child.py INPUT.npz OUTPUT.npz SYSTEM[,SYSTEM...] [refuse]

Every named system of INPUT (written by the parent from tests/sparse_solve_ref.py and tests/sparse_sigma_ref.py) is
analyzed in MODE_SPARSE. Per system, in the layout of vals:
  base     the existing path (sar.baseline_columns, one spp_factor_solve_device per column) on the unit columns of the
           checked vertices, read at the rows of the column's stored blocks (NaN elsewhere)
  solve    spp_sparse_solve_device on all n unit columns in passes of 128, read at the same rows
  sigma    spp_sparse_sigma_device into a NaN-filled buffer between NaN guards; sigma2 a second call
and beside them the solves before and after the call, spp_factor_solve_device(eta) after it and on a ctx that never made
it, the flags, the front table, sparse_block_diagonal() and sparse_marginals([v]) of the selected vertices. `refuse`: the
refusals as well. This process asserts return codes of the healthy calls only; everything else is the parent's."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from slam_plus_plus_amd import api  # noqa: E402
import solve_again_ref as sar  # noqa: E402
import sparse_sigma_ref as sgr  # noqa: E402
from slam_plus_plus_amd.blockcsc import BlockCSC  # noqa: E402
from sparse_solve_child import FRONT_KEYS, factor, framed_solve  # noqa: E402

GUARD = 8       # NaN doubles in front of and behind d_sigma
PASS = 128


def system(inp, name):
    g = lambda k: inp["%s/%s" % (name, k)]  # noqa: E731
    return BlockCSC(g("dim"), g("col_ptr"), g("row_idx"), g("blk_off"), g("vals")), g("eta")


def framed_sigma(c, nvals):
    """spp_sparse_sigma_device into the middle of a NaN-filled buffer: (sigma, whether both guards are untouched)"""
    d = api.DeviceArray.from_host(c, np.full(nvals + 2 * GUARD, np.nan))
    assert c.sparse_sigma_device(d.ptr + 8 * GUARD) == 0
    out = d.download()
    d.free()
    return out[GUARD:GUARD + nvals].copy(), bool(np.all(np.isnan(out[:GUARD])) and np.all(np.isnan(out[GUARD + nvals:])))


def solve_route(c, lam, index):
    """Sigma on the pattern from spp_sparse_solve_device on all n unit columns, in passes of 128"""
    pos, r, col, _ = index
    out = np.full(lam.nvals, np.nan)
    n = lam.n
    for k0 in range(0, n, PASS):
        kc = min(PASS, n - k0)
        E = np.zeros((n, kc), order="F")
        E[k0 + np.arange(kc), np.arange(kc)] = 1.0
        d = api.DeviceArray.from_host(c, E.ravel(order="F"))
        assert c.sparse_solve_device(d.ptr, kc, n) == 0
        X = d.download().reshape((n, kc), order="F")
        d.free()
        m = (col >= k0) & (col < k0 + kc)
        out[pos[m]] = X[r[m], col[m] - k0]
    return out


def one_system(inp, out, name):
    lam, eta = system(inp, name)
    check = inp[name + "/check"]
    sel = inp[name + "/sel"]
    index = sgr.pattern_index(lam)
    pos, r, col, _ = index
    c = api.Context(0)
    c.analyze(lam, api.MODE_SPARSE)
    dv = api.DeviceArray.from_host(c, lam.vals)
    # the existing path on the unit columns of the checked vertices
    E, rows = sar.unit_columns(lam, check)
    Xb = sar.baseline_columns(c, dv.ptr, E)
    at = np.full(lam.n, -1, dtype=np.int64)
    at[rows] = np.arange(rows.size)
    base = np.full(lam.nvals, np.nan)
    m = at[col] >= 0
    base[pos[m]] = Xb[r[m], at[col[m]]]
    out[name + "/base"] = base
    st, x_eta = factor(c, dv, eta)
    assert st == 0
    out[name + "/x_eta"] = x_eta
    kept = [c.info("SPARSE_FACTOR_KEPT")]
    out[name + "/solve"] = solve_route(c, lam, index)
    B = np.stack([eta, np.arange(1.0, lam.n + 1.0)], axis=1)
    out[name + "/X_before"], _ = framed_solve(c, B)
    frames = []
    out[name + "/sigma"], ok = framed_sigma(c, lam.nvals)
    frames.append(ok)
    kept += [c.info("SPARSE_FACTOR_KEPT"), c.info("FACTOR_KEPT")]
    out[name + "/X_after"], _ = framed_solve(c, B)
    out[name + "/sigma2"], ok = framed_sigma(c, lam.nvals)
    frames.append(ok)
    out[name + "/frames"] = np.array(frames)
    out[name + "/sigma_host"] = c.sparse_sigma()
    diag = c.sparse_block_diagonal()
    out[name + "/n_diag"] = np.int64(len(diag))
    for v in sel:
        out["%s/diag%d" % (name, v)] = diag[int(v)]
        out["%s/marg%d" % (name, v)] = c.sparse_marginals([int(v)])
    kept.append(c.info("SPARSE_FACTOR_KEPT"))
    st, out[name + "/x_eta_after"] = factor(c, dv, eta)
    assert st == 0
    out[name + "/kept"] = np.array(kept)
    fr = c.sparse_fronts()
    for k in FRONT_KEYS:
        out["%s/front_%s" % (name, k)] = fr[k]
    dv.free()
    c.close()
    # a ctx that never made the call: spp_factor_solve_device gives the same bits
    c = api.Context(0)
    c.analyze(lam, api.MODE_SPARSE)
    dv = api.DeviceArray.from_host(c, lam.vals)
    st, out[name + "/x_eta_fresh"] = factor(c, dv, eta)
    assert st == 0
    dv.free()
    c.close()


class Refusals:
    def __init__(self, out):
        self.out, self.tags = out, []

    def probe(self, tag, c, nvals):
        """the call with valid arguments on a ones-filled d_sigma: (code, d_sigma intact, SPARSE_FACTOR_KEPT)"""
        dS = api.DeviceArray.from_host(c, np.ones(nvals))
        code = c.lib.spp_sparse_sigma_device(c.h, dS.ptr)
        kept = ctypes.c_int64(-1)
        assert c.lib.spp_get_info(c.h, api.INFO["SPARSE_FACTOR_KEPT"], ctypes.byref(kept)) == 0
        self.record(tag, [code], np.array_equal(dS.download(), np.ones(nvals)), kept.value)
        dS.free()

    def record(self, tag, codes, intact, kept):
        self.tags.append(tag)
        self.out["refuse/%s" % tag] = np.array(list(codes) + [int(intact), int(kept)], dtype=np.int64)

    def usable(self, tag, c, lam, eta, dv, ref_sigma):
        """the ctx factors, keeps the factor and inverts: the largest difference from the sigma of the healthy run"""
        st, _ = factor(c, dv, eta)
        kept = c.info("SPARSE_FACTOR_KEPT")
        sigma, ok = framed_sigma(c, lam.nvals)
        self.out["usable/%s" % tag] = np.array([st, kept, int(ok), float(np.abs(sigma - ref_sigma).max() / np.abs(ref_sigma).max())])


def refusals(inp, out):
    R = Refusals(out)
    lam, eta = system(inp, "forest_a")
    ref_sigma = out["forest_a/sigma"]
    nv = lam.nvals
    c = api.Context(0)
    dv = api.DeviceArray.from_host(c, lam.vals)
    R.probe("state:before_analyze", c, nv)
    c.analyze(lam, api.MODE_SPARSE)
    R.probe("state:before_factor", c, nv)
    R.usable("after_first_refusals", c, lam, eta, dv, ref_sigma)
    # a designed negative pivot (the class-2 clique of forest_a): SPP_NOT_POSDEF keeps nothing
    vals = lam.vals.copy()
    vals[int(inp["fail_offset"])] = float(inp["fail_value"])
    dbad = api.DeviceArray.from_host(c, vals)
    out["fail/status"] = np.int64(factor(c, dbad, eta)[0])
    dbad.free()
    R.probe("state:after_not_posdef", c, nv)
    R.usable("after_not_posdef", c, lam, eta, dv, ref_sigma)
    # a null pointer: refused, the factor stays kept
    dS = api.DeviceArray.from_host(c, np.ones(nv))
    codes = [c.lib.spp_sparse_sigma_device(c.h, None), c.lib.spp_sparse_sigma_device(None, dS.ptr)]
    R.record("badarg", codes, np.array_equal(dS.download(), np.ones(nv)), c.info("SPARSE_FACTOR_KEPT"))
    dS.free()
    R.usable("after_badarg", c, lam, eta, dv, ref_sigma)
    c.analyze(lam, api.MODE_SPARSE)
    R.probe("state:after_analyze", c, nv)
    R.usable("after_analyze", c, lam, eta, dv, ref_sigma)
    A = np.eye(5) * 3.0
    dA, db = api.DeviceArray.from_host(c, A.ravel()), api.DeviceArray.from_host(c, np.ones(5))
    assert c._check(c.lib.spp_dense_posv(c.h, dA.ptr, 5, 5, db.ptr)) == 0
    dA.free(); db.free()
    R.probe("state:after_dense_posv", c, nv)
    R.usable("after_dense_posv", c, lam, eta, dv, ref_sigma)
    c.set_shard(0, 2)
    R.probe("unsupported:sharded", c, nv)
    c.set_shard(0, 1)
    R.probe("state:after_set_shard", c, nv)
    R.usable("after_set_shard", c, lam, eta, dv, ref_sigma)
    c.lib.spp_free_memory(c.h)
    R.probe("state:after_free_memory", c, nv)
    dv.free()
    c.close()
    # SPP_MODE_AUTO resolving to the sparse mode keeps the factor too
    c = api.Context(0)
    c.analyze(lam, api.MODE_AUTO)
    dv = api.DeviceArray.from_host(c, lam.vals)
    out["auto/mode"] = np.int64(c.info("MODE"))
    R.usable("auto", c, lam, eta, dv, ref_sigma)
    dv.free()
    c.close()
    # the Schur modes: unsupported after a healthy factor of their own
    for tag, name, mode in (("schur", "edges73_aligned", api.MODE_SCHUR), ("schur_sparse", "edges73_aligned", api.MODE_SCHUR_SPARSE),
                            ("schur_mis", "mis33", api.MODE_SCHUR_MIS)):
        slam, seta = sar.problem(name)
        c = api.Context(0)
        c.analyze(slam, mode)
        dv = api.DeviceArray.from_host(c, slam.vals)
        assert factor(c, dv, seta)[0] == 0
        R.probe("unsupported:" + tag, c, slam.nvals)
        st, x = factor(c, dv, seta)          # the ctx goes on solving in its own mode
        out["usable/" + tag] = np.array([st, float(np.linalg.norm(slam.matvec(x) - seta) / np.linalg.norm(seta))])
        dv.free()
        c.close()
    out["refuse_tags"] = np.array(R.tags)


def main():
    inp = np.load(sys.argv[1])
    out = {}
    for name in sys.argv[3].split(","):
        one_system(inp, out, name)
    if "refuse" in sys.argv[4:]:
        refusals(inp, out)
    np.savez(sys.argv[2], **out)
    print("ok: %d arrays" % len(out))


if __name__ == "__main__":
    main()
