"""Child process of tests/test_gpu_solve_again_schedules.py: the library reads its switches once per process, so every
variant is one run of this file with the switches in its environment.

    python solve_again_child.py INPUT.npz OUTPUT.npz FIXTURE[,FIXTURE...] [sequence]

Every named system of INPUT (written by the parent from tests/solve_again_ref.py: Lambda, eta, B, the selected vertices and
their rows, other values on the same structure) is analyzed in MODE_SCHUR. Per system, in one context: the existing
path on every column of B and on every unit column of the selection (one spp_factor_solve_device each: the yardstick's
reference backend under the same switches), then spp_factor_solve_device(eta), what it left (the SPP_INFO words, the own S
buffer, the ordering), spp_solve_device on NaN-framed copies of the leading 1, 6, 17 (and all, where B has more) columns,
single columns, a repeat, the joint covariance of the selection, twice, single vertices alone, and
spp_factor_solve_device(eta) again.

`sequence`: the zero-tile invariant as the solves see it. Values A, B, A, a non-positive pivot, B in ONE context with a
6-column solve behind every good factor and both entry points behind the bad one; a larger system and then a smaller one with
another mask analyzed in one context. Every solve is compared (numpy.array_equal) with the same solve of a fresh context.

This process computes no reference and asserts the return codes of the healthy calls only; everything else is the parent's."""
import ctypes
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from slam_plus_plus_amd import api  # noqa: E402
from slam_plus_plus_amd.blockcsc import BlockCSC  # noqa: E402

INFO_WORDS = ("DENSE_STREAMED", "S_CLEAR", "LM_STREAM", "SCHUR_SIDE", "SOLVE_ASYNC", "FACTOR_KEPT", "S_LD", "N_REDUCED", "N_POSES")
ALONE = (0, 15, 16, 127, 128)
K_SEQ = 6
SEQ_ANALYZE = ("loop73", "chain73")   # the larger system first, then the smaller one in its buffers


def framed_solve(c, dv, B, ldb=None, extra_cols=1):
    """spp_solve_device on a NaN-framed copy of B: (the n x k result, whether the frame is untouched)"""
    n, k = B.shape
    ldb = n + 3 if ldb is None else ldb
    buf = np.full((ldb, k + extra_cols), np.nan, order="F")
    buf[:n, :k] = B
    dB = api.DeviceArray.from_host(c, buf.ravel(order="F"))
    assert c.solve_device(dv.ptr, dB.ptr, k, ldb) == 0
    out = dB.download().reshape((ldb, k + extra_cols), order="F")   # (the download is ordered behind the solve)
    dB.free()
    return out[:n, :k].copy(), bool(np.all(np.isnan(out[n:, :])) and np.all(np.isnan(out[:, k:])))


def factor(c, dv, eta):
    dr = api.DeviceArray.from_host(c, eta)
    st = c.factor_solve_device(dv.ptr, dr.ptr)
    x = dr.download()
    dr.free()
    return st, x


def own_S(c):
    """the S | rhs buffer spp_factor_solve_device owns (as tests/test_gpu_solve_again.py reads it)"""
    out = np.empty(c.schur_buffer_size())
    c._check(c.lib.spp_memcpy_d2h(c.h, out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(c.info("S_DEVICE_PTR")), out.nbytes))
    return out


def info_words(c):
    return np.array([c.info(k) for k in INFO_WORDS], dtype=np.int64)


def system(inp, name):
    g = lambda k: inp["%s/%s" % (name, k)]  # noqa: E731
    return BlockCSC(g("dim"), g("col_ptr"), g("row_idx"), g("blk_off"), g("vals")), g("eta")


def designed(inp, out, name):
    lam, eta = system(inp, name)
    B, sel, alone_v, rows = (inp["%s/%s" % (name, k)] for k in ("B", "sel", "sel_alone", "rows"))
    E = np.zeros((lam.n, rows.size))
    E[rows, np.arange(rows.size)] = 1.0          # the unit columns of the selection's rows
    c = api.Context(0)
    c.analyze(lam, api.MODE_SCHUR)
    dv = api.DeviceArray.from_host(c, lam.vals)
    kept = [c.info("FACTOR_KEPT")]
    base = np.empty_like(B)
    for j in range(B.shape[1]):
        st, base[:, j] = factor(c, dv, np.ascontiguousarray(B[:, j]))
        assert st == 0
        if j == 0:
            out[name + "/info_first"] = info_words(c)
    out[name + "/base"] = base
    base_e = np.empty((rows.size, E.shape[1]))
    for j in range(E.shape[1]):
        st, x = factor(c, dv, np.ascontiguousarray(E[:, j]))
        assert st == 0
        base_e[:, j] = x[rows]
    out[name + "/base_cov"] = base_e
    st, x_eta = factor(c, dv, eta)
    assert st == 0
    kept.append(c.info("FACTOR_KEPT"))
    out[name + "/x_eta"] = x_eta
    out[name + "/info"] = info_words(c)
    S = own_S(c)
    out[name + "/S_sha"] = np.frombuffer(hashlib.sha256(S.tobytes()).digest(), dtype=np.uint8)
    out[name + "/S_nan"] = np.int64(np.count_nonzero(np.isnan(S)))
    del S
    out[name + "/ordering"] = c.ordering(lam.nb)
    frames = []
    kmax = B.shape[1]
    for k in (1, 6, 17) + ((kmax,) if kmax > 17 else ()):
        out["%s/X%d" % (name, k)], ok = framed_solve(c, dv, B[:, :k])
        frames.append(ok)
    for j in ALONE:
        if j < kmax:
            out["%s/alone%d" % (name, j)], ok = framed_solve(c, dv, B[:, j:j + 1])
            frames.append(ok)
    out[name + "/again"], ok = framed_solve(c, dv, B[:, :17], ldb=lam.n, extra_cols=2)
    frames.append(ok)
    kept.append(c.info("FACTOR_KEPT"))
    out[name + "/frames"] = np.array(frames)
    out[name + "/cov"] = c.marginals(dv.ptr, sel)
    for v in alone_v:
        out["%s/cov_alone%d" % (name, v)] = c.marginals(dv.ptr, [int(v)])
    out[name + "/cov_again"] = c.marginals(dv.ptr, sel)
    kept.append(c.info("FACTOR_KEPT"))
    st, out[name + "/x_eta_after"] = factor(c, dv, eta)
    assert st == 0
    kept.append(c.info("FACTOR_KEPT"))
    out[name + "/kept"] = np.array(kept, dtype=np.int64)
    dv.free()
    c.close()


def refused(c, dv, n):
    """both entry points on a ones-filled B: (the two return codes, B intact, FACTOR_KEPT)"""
    dB = api.DeviceArray.from_host(c, np.ones(n))
    dC = api.DeviceArray(c, 64)
    v = np.zeros(1, dtype=np.int64)
    codes = [c.lib.spp_solve_device(c.h, dv.ptr, dB.ptr, n, 1),
             c.lib.spp_marginals_device(c.h, dv.ptr, 1, v.ctypes.data_as(ctypes.c_void_p), dC.ptr)]
    intact = np.array_equal(dB.download(), np.ones(n))
    kept = ctypes.c_int64(-1)
    assert c.lib.spp_get_info(c.h, api.INFO["FACTOR_KEPT"], ctypes.byref(kept)) == 0
    dB.free(); dC.free()
    return np.array(codes + [int(intact), kept.value], dtype=np.int64)


def fresh_solve(lam, vals, eta, B):
    """factor and solve of a context that has seen nothing else: (x, X)"""
    c = api.Context(0)
    c.analyze(lam, api.MODE_SCHUR)
    dv = api.DeviceArray.from_host(c, vals)
    st, x = factor(c, dv, eta)
    assert st == 0
    X, ok = framed_solve(c, dv, B)
    assert ok
    dv.free()
    c.close()
    return x, X


def sequence(inp, out, names):
    for name in names:
        lam, eta = system(inp, name)
        B = inp[name + "/B"][:, :K_SEQ]
        vals = {"A": lam.vals, "B": inp[name + "/vals_b"]}
        want = {k: fresh_solve(lam, v, eta, B) for k, v in vals.items()}
        assert not np.array_equal(want["A"][1], want["B"][1])
        c = api.Context(0)
        c.analyze(lam, api.MODE_SCHUR)
        dv = api.DeviceArray(c, lam.vals.size)
        equal, clear = [], []
        for step in ("A", "B", "A", "bad", "B"):
            if step == "bad":
                dv.upload(inp[name + "/vals_bad"])
                out["seq/%s/bad_code" % name] = np.int64(factor(c, dv, eta)[0])
                out["seq/%s/refused" % name] = refused(c, dv, lam.n)
                continue
            dv.upload(vals[step])
            st, x = factor(c, dv, eta)
            clear.append(c.info("S_CLEAR"))
            X, ok = framed_solve(c, dv, B)
            equal.append(bool(st == 0 and ok and np.array_equal(x, want[step][0]) and np.array_equal(X, want[step][1])))
        out["seq/%s/equal" % name] = np.array(equal)
        out["seq/%s/clear" % name] = np.array(clear, dtype=np.int64)
        dv.free()
        c.close()
    # one context analyzed for the larger system, then for the smaller one: another mask in the same buffers
    c = api.Context(0)
    equal = []
    for name in SEQ_ANALYZE:
        lam, eta = system(inp, name)
        B = inp[name + "/B"][:, :K_SEQ]
        want = fresh_solve(lam, lam.vals, eta, B)
        c.analyze(lam, api.MODE_SCHUR)
        dv = api.DeviceArray.from_host(c, lam.vals)
        st, x = factor(c, dv, eta)
        X, ok = framed_solve(c, dv, B)
        equal.append(bool(st == 0 and ok and np.array_equal(x, want[0]) and np.array_equal(X, want[1])))
        dv.free()
    c.close()
    out["seq/analyze/equal"] = np.array(equal)
    out["seq/names"] = np.array(list(names))


def main():
    inp = np.load(sys.argv[1])
    out = {"env": np.array(sorted("%s=%s" % kv for kv in os.environ.items() if kv[0].startswith("SPP_") and kv[0] != "SPP_LIB"))}
    names = sys.argv[3].split(",")
    for name in names:
        designed(inp, out, name)
    if "sequence" in sys.argv[4:]:
        sequence(inp, out, [str(s) for s in inp["sequence_names"]])
    np.savez(sys.argv[2], **out)
    print("ok: %d arrays" % len(out))


if __name__ == "__main__":
    main()
