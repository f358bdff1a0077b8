"""Child process of tests/test_gpu_sparse_solve_again.py: the library reads its switches once per process, so every variant
is one run of this file with the switches in its environment.

    python sparse_solve_child.py INPUT.npz OUTPUT.npz FIXTURE[,FIXTURE...] [refuse]

Every named system of INPUT (written by the parent from tests/sparse_solve_ref.py) is analyzed in MODE_SPARSE. Per system:
the existing path on every column of B (one spp_factor_solve_device each: the yardstick's reference backend), then
spp_factor_solve_device(eta) and spp_sparse_solve_device on NaN-framed copies of the leading 1, 6, 17 (tree_hi: 129) columns,
a repeat, single columns, and spp_factor_solve_device(eta) again. `refuse`: the refusals as well, each recorded as
(return codes, B intact, SPARSE_FACTOR_KEPT before / after). This process asserts return codes of the healthy calls only;
everything else is the parent's."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from slam_plus_plus_amd import api  # noqa: E402
from slam_plus_plus_amd.blockcsc import BlockCSC  # noqa: E402

FRONT_KEYS = ("h", "w", "pad", "cls", "level", "parent", "team")
ALONE = (0, 15, 16, 127, 128)


def framed_solve(c, B, ldb=None, extra_cols=1):
    """spp_sparse_solve_device on a NaN-framed copy of B: (the n x k result, whether the frame is untouched)"""
    n, k = B.shape
    ldb = n + 3 if ldb is None else ldb
    buf = np.full((ldb, k + extra_cols), np.nan, order="F")
    buf[:n, :k] = B
    dB = api.DeviceArray.from_host(c, buf.ravel(order="F"))
    assert c.sparse_solve_device(dB.ptr, k, ldb) == 0
    out = dB.download().reshape((ldb, k + extra_cols), order="F")   # (the download is ordered behind the solve)
    dB.free()
    return out[:n, :k].copy(), bool(np.all(np.isnan(out[n:, :])) and np.all(np.isnan(out[:, k:])))


def factor(c, dv, eta):
    dr = api.DeviceArray.from_host(c, eta)
    st = c.factor_solve_device(dv.ptr, dr.ptr)
    x = dr.download()
    dr.free()
    return st, x


def system(inp, name):
    g = lambda k: inp["%s/%s" % (name, k)]  # noqa: E731
    return BlockCSC(g("dim"), g("col_ptr"), g("row_idx"), g("blk_off"), g("vals")), g("eta"), g("B")


def designed(inp, out, name):
    lam, eta, B = system(inp, name)
    c = api.Context(0)
    c.analyze(lam, api.MODE_SPARSE)
    dv = api.DeviceArray.from_host(c, lam.vals)
    base = np.empty_like(B)
    for j in range(B.shape[1]):
        st, base[:, j] = factor(c, dv, np.ascontiguousarray(B[:, j]))
        assert st == 0
    out[name + "/base"] = base
    kept = [c.info("SPARSE_FACTOR_KEPT")]
    st, x_eta = factor(c, dv, eta)
    assert st == 0
    kept.append(c.info("SPARSE_FACTOR_KEPT"))
    out[name + "/x_eta"] = x_eta
    frames = []
    for k in (1, 6, 17) + ((B.shape[1],) if B.shape[1] > 17 else ()):
        out["%s/X%d" % (name, k)], ok = framed_solve(c, B[:, :k])
        frames.append(ok)
    kmax = B.shape[1]
    out[name + "/again"], ok = framed_solve(c, B, ldb=lam.n, extra_cols=2)
    frames.append(ok)
    for j in ALONE:
        if j < kmax:
            out["%s/alone%d" % (name, j)], ok = framed_solve(c, B[:, j:j + 1])
            frames.append(ok)
    kept.append(c.info("SPARSE_FACTOR_KEPT"))
    out[name + "/frames"] = np.array(frames)
    st, out[name + "/x_eta_after"] = factor(c, dv, eta)
    assert st == 0
    out[name + "/kept"] = np.array(kept + [c.info("FACTOR_KEPT")])
    fr = c.sparse_fronts()
    for k in FRONT_KEYS:
        out["%s/front_%s" % (name, k)] = fr[k]
    dv.free()
    c.close()
    # a ctx that never solved again: spp_factor_solve_device gives the same bits
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

    def probe(self, tag, c, n):
        """both calls with valid arguments on a ones-filled B: (codes, B intact, SPARSE_FACTOR_KEPT)"""
        dB = api.DeviceArray.from_host(c, np.ones(n))
        dC = api.DeviceArray(c, 64)
        v = np.zeros(1, dtype=np.int64)
        codes = [c.lib.spp_sparse_solve_device(c.h, dB.ptr, n, 1),
                 c.lib.spp_sparse_marginals_device(c.h, 1, v.ctypes.data_as(ctypes.c_void_p), dC.ptr)]
        kept = ctypes.c_int64(-1)
        assert c.lib.spp_get_info(c.h, api.INFO["SPARSE_FACTOR_KEPT"], ctypes.byref(kept)) == 0
        self.record(tag, codes, np.array_equal(dB.download(), np.ones(n)), kept.value)
        dB.free(); dC.free()

    def record(self, tag, codes, intact, kept):
        self.tags.append(tag)
        self.out["refuse/%s" % tag] = np.array(list(codes) + [int(intact), int(kept)], dtype=np.int64)

    def usable(self, tag, c, lam, eta, dv):
        """the ctx factors, keeps the factor and solves again: the residual of that solve"""
        st, _ = factor(c, dv, eta)
        kept = c.info("SPARSE_FACTOR_KEPT")
        X, ok = framed_solve(c, eta[:, None])
        res = float(np.linalg.norm(lam.matvec(X[:, 0]) - eta) / np.linalg.norm(eta))
        self.out["usable/%s" % tag] = np.array([st, kept, int(ok), res])


def refusals(inp, out):
    import solve_again_ref as sar
    R = Refusals(out)
    lam, eta, _ = system(inp, "forest_a")
    n = lam.n
    c = api.Context(0)
    dv = api.DeviceArray.from_host(c, lam.vals)
    R.probe("state:before_analyze", c, n)
    c.analyze(lam, api.MODE_SPARSE)
    R.probe("state:before_factor", c, n)
    R.usable("after_first_refusals", c, lam, eta, dv)
    # a designed negative pivot (the class-2 clique of forest_a): SPP_NOT_POSDEF keeps nothing
    vals = lam.vals.copy()
    vals[int(inp["fail_offset"])] = float(inp["fail_value"])
    dbad = api.DeviceArray.from_host(c, vals)
    out["fail/status"] = np.int64(factor(c, dbad, eta)[0])
    dbad.free()
    R.probe("state:after_not_posdef", c, n)
    R.usable("after_not_posdef", c, lam, eta, dv)
    # spp_solve_device / spp_marginals_device on the same sparse ctx: unsupported, and they keep the sparse factor
    dB = api.DeviceArray.from_host(c, np.ones(n))
    dC = api.DeviceArray(c, 64)
    v = np.zeros(1, dtype=np.int64)
    codes = [c.lib.spp_solve_device(c.h, dv.ptr, dB.ptr, n, 1),
             c.lib.spp_marginals_device(c.h, dv.ptr, 1, v.ctypes.data_as(ctypes.c_void_p), dC.ptr)]
    R.record("dense_calls_on_sparse_ctx", codes, np.array_equal(dB.download(), np.ones(n)), c.info("SPARSE_FACTOR_KEPT"))
    # bad arguments: refused, the factor stays kept
    lib, h = c.lib, c.h

    def marg(vs, cov=dC.ptr):
        vs = np.asarray(vs, dtype=np.int64)
        return lib.spp_sparse_marginals_device(h, vs.size, vs.ctypes.data_as(ctypes.c_void_p), cov)
    codes = [lib.spp_sparse_solve_device(h, dB.ptr, n, 0), lib.spp_sparse_solve_device(h, dB.ptr, n - 1, 1),
             lib.spp_sparse_solve_device(h, None, n, 1), marg([0, 1, 0]), marg([lam.nb]), marg([-1]),
             lib.spp_sparse_marginals_device(h, 0, v.ctypes.data_as(ctypes.c_void_p), dC.ptr),
             lib.spp_sparse_marginals_device(h, 1, None, dC.ptr), marg([0], None)]
    R.record("badarg", codes, np.array_equal(dB.download(), np.ones(n)), c.info("SPARSE_FACTOR_KEPT"))
    dB.free(); dC.free()
    R.usable("after_badarg", c, lam, eta, dv)
    c.analyze(lam, api.MODE_SPARSE)
    R.probe("state:after_analyze", c, n)
    R.usable("after_analyze", c, lam, eta, dv)
    A = np.eye(5) * 3.0
    dA, db = api.DeviceArray.from_host(c, A.ravel()), api.DeviceArray.from_host(c, np.ones(5))
    assert c._check(c.lib.spp_dense_posv(c.h, dA.ptr, 5, 5, db.ptr)) == 0
    dA.free(); db.free()
    R.probe("state:after_dense_posv", c, n)
    R.usable("after_dense_posv", c, lam, eta, dv)
    c.set_shard(0, 2)
    R.probe("unsupported:sharded", c, n)
    c.set_shard(0, 1)
    R.probe("state:after_set_shard", c, n)
    R.usable("after_set_shard", c, lam, eta, dv)
    c.lib.spp_free_memory(c.h)
    R.probe("state:after_free_memory", c, n)
    dv.free()
    c.close()
    # SPP_MODE_AUTO resolving to the sparse mode keeps the factor too
    c = api.Context(0)
    c.analyze(lam, api.MODE_AUTO)
    dv = api.DeviceArray.from_host(c, lam.vals)
    out["auto/mode"] = np.int64(c.info("MODE"))
    R.usable("auto", c, lam, eta, dv)
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
        R.probe("unsupported:" + tag, c, slam.n)
        st, x = factor(c, dv, seta)          # the ctx goes on solving in its own mode
        out["usable/" + tag] = np.array([st, float(np.linalg.norm(slam.matvec(x) - seta) / np.linalg.norm(seta))])
        dv.free()
        c.close()
    out["refuse_tags"] = np.array(R.tags)


def main():
    inp = np.load(sys.argv[1])
    out = {}
    for name in sys.argv[3].split(","):
        designed(inp, out, name)
    if "refuse" in sys.argv[4:]:
        refusals(inp, out)
    np.savez(sys.argv[2], **out)
    print("ok: %d arrays" % len(out))


if __name__ == "__main__":
    main()
