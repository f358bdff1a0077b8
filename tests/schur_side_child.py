"""Child process of tests/test_gpu_schur_side.py and tests/test_gpu_schur_clear.py (the switches of the library are read
once per process, so every variant runs in a process of its own). Prints one line "RESULT <json>".

  side  <refs.pkl> <json options>   the edge fixtures of tests/schur_fixtures.py and edges73: S | rhs formed twice and solved twice in
                                    one context (bit-reproducible), checked against the longdouble reference, then two
                                    landmark shards on one device through the split API (edges63, edges73); sha256 of
                                    everything
  clear <problem> <json options>    values A, B, A solved in ONE context, each compared with a fresh context's solve of the
                                    same values; then a failed pivot followed by a good solve; what schur_form cleared each
                                    time; which tiles of the solver's S buffer hold anything afterwards"""
import ctypes
import hashlib
import json
import os
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from slam_plus_plus_amd import api, synth  # noqa: E402
import schur_fixtures as fx  # noqa: E402
import schur_fixtures_73 as fx73  # noqa: E402

NB = 128
SIDE_CASES = [("edges63", api.MODE_SCHUR), ("edges63_long", api.MODE_SCHUR), ("edges32", api.MODE_SCHUR),
              ("mis66", api.MODE_SCHUR_MIS), ("edges73", api.MODE_SCHUR)]
SHARD_CASES = ["edges63", "edges73"]   # two landmark shards each, reported as "<name>/2 shards"


def chain90():
    """an open chain of 90 six-wide cameras, every point seen by three consecutive cameras: S is a band of 5 tile rows
    (n_red = 540) in which tiles (0, 2), (0, 3) and (1, 3) stay empty"""
    nc = 90
    obs = []
    lm = 0
    for c in range(nc - 2):
        for _ in range(4):
            obs += [(c, lm), (c + 1, lm), (c + 2, lm)]
            lm += 1
    return fx._guided(nc, lm, 6, 3, obs, [], 90)


def problem(name):
    if name == "chain90":
        return chain90()
    if name == "ba_ring300":   # the ring of tests/test_gpu_dense_tilemask.py: 15 tile rows
        from oracle import spp_oracle as orc
        return orc.assemble(synth.ba_problem(300, 20000, 100000, 300, heavy_tail=True, name=name))
    return fx73.make_any(name)   # (chain73: 6 tile rows, loop73: 19, 7-wide cameras that straddle the tile boundaries)


def diagonal_entries(lam):
    """index in vals of every diagonal entry of every diagonal block"""
    idx = []
    for j in range(lam.nb):
        p = lam.col_ptr[j + 1] - 1
        assert lam.row_idx[p] == j
        d = int(lam.dim[j])
        idx.append(lam.blk_off[p] + np.arange(d) * (d + 1))
    return np.concatenate(idx)


def values_b(lam):
    """other values on the same structure, still positive definite: 1.5 Lambda + 0.7 I"""
    v = 1.5 * lam.vals
    v[diagonal_entries(lam)] += 0.7
    return v


def values_bad(lam):
    """a camera (the widest block width) whose diagonal block is far from positive: S has a non-positive pivot"""
    v = lam.vals.copy()
    cam = int(np.flatnonzero(lam.dim == lam.dim.max())[7])
    p = lam.col_ptr[cam + 1] - 1
    d = int(lam.dim[cam])
    v[lam.blk_off[p] + np.arange(d) * (d + 1)] = -1e6
    return v


def own_s_buffer(ctx):
    """the S | rhs buffer spp_factor_solve_device owns, as an ld x ld matrix"""
    ld = ctx.info("S_LD")
    out = np.empty(ld * ld)
    ctx._check(ctx.lib.spp_memcpy_d2h(ctx.h, out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(ctx.info("S_DEVICE_PTR")),
                                      out.nbytes))
    return out.reshape((ld, ld), order="F")


def nonzero_tiles(S):
    """tiles of the upper triangle that hold anything (below it the accumulation assigns the lower halves of the diagonal
    blocks that straddle a tile edge: never an operand, never cleared)"""
    t = S.shape[0] // NB
    return sorted((i, j) for i in range(t) for j in range(i, t) if S[NB * i:NB * (i + 1), NB * j:NB * (j + 1)].any())


def solve(ctx, dv, dr, vals, eta):
    dv.upload(vals)
    dr.upload(eta)
    code = ctx.factor_solve_device(dv.ptr, dr.ptr)
    return code, dr.download(), ctx.info("S_CLEAR"), ctx.info("DENSE_STREAMED"), ctx.info("SCHUR_SIDE")


def fresh(lam, mode, vals, eta):
    ctx = api.Context(0, 0)
    ctx.analyze(lam, mode)
    dv = api.DeviceArray(ctx, lam.vals.size)
    dr = api.DeviceArray(ctx, lam.n)
    code, x, clear, _, _ = solve(ctx, dv, dr, vals, eta)
    assert code == 0 and clear in (0, 2), (code, clear)   # a new buffer is never cleared by tiles
    dv.free()
    dr.free()
    ctx.close()
    return x


def run_clear(name, opt):
    lam, eta = problem(name)
    mode = api.MODE_SCHUR
    A, B = lam.vals.copy(), values_b(lam)
    xa, xb = fresh(lam, mode, A, eta), fresh(lam, mode, B, eta)
    assert not np.array_equal(xa, xb)
    ctx = api.Context(0, 0)
    ctx.analyze(lam, mode)
    dv = api.DeviceArray(ctx, lam.vals.size)
    dr = api.DeviceArray(ctx, lam.n)
    out = dict(equal=[], clear=[], streamed=[], side=[], tile_rows=-(-ctx.info("N_REDUCED") // NB))
    tiles = []

    def step(vals, want, tag):
        code, x, clear, streamed, side = solve(ctx, dv, dr, vals, eta)
        out["equal"].append([tag, bool(code == 0 and np.array_equal(x, want))])
        out["clear"].append(clear)
        out["streamed"].append(streamed)
        out["side"].append(side)
        tiles.append(nonzero_tiles(own_s_buffer(ctx)))

    step(A, xa, "A")
    step(B, xb, "B")
    step(A, xa, "A again")
    # a non-positive pivot, then a good solve: the status reset is not lost, nothing of the failed factor stays behind
    code, _, clear, _, _ = solve(ctx, dv, dr, values_bad(lam), eta)
    out["bad_code"] = code
    out["clear"].append(clear)
    step(B, xb, "B after the failed pivot")
    if opt.get("posv"):
        # another factorization on the same context between two streamed solves (spp_dense_posv_masked works on a buffer of
        # its own, the per-step path below SPP_TAIL_ROWS included: the API reaches the solver's S buffer through
        # spp_factor_solve_device alone)
        n = 300
        rng = np.random.default_rng(5)
        M = rng.standard_normal((n, n))
        M = M @ M.T + n * np.eye(n)
        dA = api.DeviceArray.from_host(ctx, np.asfortranarray(M).reshape(-1, order="F"))
        db = api.DeviceArray.from_host(ctx, rng.standard_normal(n))
        assert ctx._check(ctx.lib.spp_dense_posv_masked(ctx.h, dA.ptr, n, n, db.ptr, None, 0)) == 0
        dA.free()
        db.free()
        step(A, xa, "A after another factorization")
    out["tiles"] = tiles
    words = api.schur_tile_mask_host(lam)
    used = bool(api.schur_cam_order_host(lam)[1]) if opt.get("cam_order", True) else False
    out["cam_order_used"] = used
    out["mask"] = [int(w) for w in words]
    dv.free()
    dr.free()
    ctx.close()
    return out


def run_side(refs_path, opt):
    import schur_ref
    refs = pickle.load(open(refs_path, "rb"))
    out = {}
    stream = None
    if opt.get("adopt"):   # torch initializes the device before the library's first context does, as in bench.py
        import torch
        torch.cuda.set_device(0)
        stream = torch.cuda.Stream()
        assert stream.cuda_stream != 0

    def context():
        ctx = api.Context(0, 0)
        if opt.get("profile"):
            ctx.set_profiling(True)
        if stream is not None:
            ctx.set_stream(stream.cuda_stream)
        return ctx

    for name, mode in SIDE_CASES:
        lam, eta = fx73.make_any(name)
        R = refs[name]
        ctx = context()
        ctx.analyze(lam, mode)
        dv = api.DeviceArray.from_host(ctx, lam.vals)
        dr = api.DeviceArray(ctx, lam.n)
        dS = api.DeviceArray(ctx, ctx.schur_buffer_size())
        bufs, xs, side = [], [], []
        for rep in range(2):
            dr.upload(eta)
            ctx.schur_form(dv.ptr, dr.ptr, dS.ptr)
            side.append(ctx.info("SCHUR_SIDE"))
            ctx.synchronize()
            bufs.append(dS.download())
            assert ctx.factor_solve_device(dv.ptr, dr.ptr) == 0
            side.append(ctx.info("SCHUR_SIDE"))
            xs.append(dr.download())
        assert np.array_equal(bufs[0], bufs[1]), "%s: S | rhs not bit-reproducible" % name
        assert np.array_equal(xs[0], xs[1]), "%s: x not bit-reproducible" % name
        rs = schur_ref.check_schur_buffer(R, bufs[0], mode != api.MODE_SCHUR, ctx.info("S_LD"))
        rl, rc = schur_ref.check_solution(R, lam, eta, xs[0])
        out[name] = dict(S=hashlib.sha256(bufs[0].tobytes()).hexdigest(), x=hashlib.sha256(xs[0].tobytes()).hexdigest(),
                         side=side, ratio_S=rs, ratio_xl=rl, ratio_xc=rc)
        for d in (dv, dr, dS):
            d.free()
        ctx.close()

    # split API: two landmark shards on one device, packed, summed on the host (the all-reduce), unpacked, finished
    for name in SHARD_CASES:
        out[name + "/2 shards"] = two_shards(context, *fx73.make_any(name))
    return out


def two_shards(context, lam, eta):
    ctxs, bufs, side = [], [], []
    hS, hx = hashlib.sha256(), hashlib.sha256()
    for r in range(2):
        c = context()
        c.set_shard(r, 2)
        c.analyze(lam, api.MODE_SCHUR)
        dv = api.DeviceArray.from_host(c, lam.vals)
        dr = api.DeviceArray.from_host(c, eta)
        dS = api.DeviceArray(c, c.schur_buffer_size())
        dP = api.DeviceArray(c, c.schur_packed_size())
        c.schur_form(dv.ptr, dr.ptr, dS.ptr)
        c.schur_pack(dS.ptr, dP.ptr)      # (no synchronization between the two: the pack reads S | rhs on the ctx stream)
        side.append(c.info("SCHUR_SIDE"))
        c.synchronize()
        ctxs.append(c)
        bufs.append((dv, dr, dS, dP))
    for b in bufs:
        hS.update(b[2].download().tobytes())
    psum = sum(b[3].download() for b in bufs)
    hS.update(psum.tobytes())
    for c, (dv, dr, dS, dP) in zip(ctxs, bufs):
        dP.upload(psum)
        c.schur_unpack(dP.ptr, dS.ptr)
        assert c.schur_finish(dv.ptr, dS.ptr, dr.ptr) == 0
        c.synchronize()
        hx.update(dr.download().tobytes())
    for c, b in zip(ctxs, bufs):
        for d in b:
            d.free()
        c.close()
    return dict(S=hS.hexdigest(), x=hx.hexdigest(), side=side)


if __name__ == "__main__":
    what, arg, opt = sys.argv[1], sys.argv[2], json.loads(sys.argv[3])
    res = run_clear(arg, opt) if what == "clear" else run_side(arg, opt)
    print("RESULT " + json.dumps(res))
