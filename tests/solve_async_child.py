"""Child process of tests/test_gpu_solve_async.py (the switches of the library are read once per process, so every value of
SPP_SOLVE_ASYNC runs in a process of its own). Usage: solve_async_child.py <out.npz> <json options>; prints one line
"RESULT <json>" and saves the solutions the parent compares with the float64 reference.

  loop300            the 300-camera loop of tests/test_gpu_cam_order.py (15 tile rows: streamed factor, chain kernel), solved
                     twice in one context
  edges63, ba_small  the edge fixture of tests/schur_fixtures.py (15 tile rows, its pair-count spread) and the smoke problem
                     (two tile rows, the shortest chain): the same
  edges73, loop73    7-wide cameras (tests/schur_fixtures_73.py): the edge fixture (17.5 tiles: the rhs column inside the
                     last tile) and the 330-camera loop (19 tile rows, its camera order accepted): the same
  six in a row       on the loop's context: two different Lambda / eta pairs alternate, six solves enqueued with no
                     synchronization between them, each result parked by a stream-ordered copy, everything downloaded at
                     the end and compared with the same solve done alone
  bad pivots         a non-positive pivot in the first tile, in arc B and in the separators: the return code, then a solve
                     on good values
  two shards         edges63 through the split API on one device (form, pack, sum, unpack, finish)
options: profile (profiling on in every context)"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from slam_plus_plus_amd import api, synth  # noqa: E402
import schur_fixtures_73 as fx73  # noqa: E402
import schur_side_child as side  # noqa: E402
import test_gpu_cam_order as loop  # noqa: E402


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def small_system(name):
    if name == "ba_small":
        from oracle import spp_oracle as orc
        return orc.assemble(synth.make("ba_small"))
    return fx73.make_any(name)


def bad_values(lam, cam):
    """the diagonal block of one camera pushed far below zero: S gets a non-positive pivot there"""
    vals = lam.vals.copy()
    p = lam.col_ptr[cam + 1] - 1
    assert lam.row_idx[p] == cam
    D = vals[lam.blk_off[p]:lam.blk_off[p] + 36].reshape(6, 6)
    D -= 10.0 * np.abs(D).max() * np.eye(6)
    return vals


def run(out_path, opt):
    out, arrays = {}, {}

    def context(lam, shard=None):
        ctx = api.Context(0, 0)
        if opt.get("profile"):
            ctx.set_profiling(True)
        if shard:
            ctx.set_shard(*shard)
        ctx.analyze(lam, api.MODE_SCHUR)
        return ctx

    def twice(name, lam, eta):
        ctx = context(lam)
        dv, dr = api.DeviceArray.from_host(ctx, lam.vals), api.DeviceArray(ctx, lam.n)
        xs, asy = [], []
        for _ in range(2):
            dr.upload(eta)
            assert ctx.factor_solve_device(dv.ptr, dr.ptr) == 0
            asy.append(ctx.info("SOLVE_ASYNC"))
            xs.append(dr.download())
        out[name] = dict(x=sha(xs[0]), repro=bool(np.array_equal(xs[0], xs[1])), asy=asy, streamed=ctx.info("DENSE_STREAMED"),
                         tile_rows=-(-ctx.info("N_REDUCED") // 128), order=ctx.ordering(lam.nb)[:ctx.info("N_POSES")].tolist())
        arrays[name.replace(" ", "_")] = xs[0]
        return ctx, dv, dr

    for name in ("edges63", "ba_small", "edges73", "loop73"):
        lam, eta = loop.system(name) if name == "loop73" else small_system(name)
        ctx, dv, dr = twice(name, lam, eta)
        dv.free()
        dr.free()
        ctx.close()

    lam, eta = loop.system("loop")
    ctx, dvA, dr = twice("loop300", lam, eta)
    xA = arrays["loop300"]

    # ---- six solves back to back, no synchronization between them
    etaB = 0.5 * eta + 1.0
    dvB = api.DeviceArray.from_host(ctx, side.values_b(lam))
    dEta = [api.DeviceArray.from_host(ctx, eta), api.DeviceArray.from_host(ctx, etaB)]
    dr.copy_from(dEta[1])
    assert ctx.factor_solve_device(dvB.ptr, dr.ptr) == 0
    ctx.synchronize()
    xB = dr.download()                      # the second pair, solved alone with a synchronization behind it
    assert not np.array_equal(xA, xB)
    park = [api.DeviceArray(ctx, lam.n) for _ in range(6)]
    codes, asy = [], []
    ctx.synchronize()
    for i in range(6):
        dr.copy_from(dEta[i % 2])
        codes.append(ctx.factor_solve_device((dvA, dvB)[i % 2].ptr, dr.ptr))
        asy.append(ctx.info("SOLVE_ASYNC"))
        park[i].copy_from(dr)               # stream-ordered, like the vertex update of a resident LM loop
    got = [p.download() for p in park]      # (the first download synchronizes)
    out["six in a row"] = dict(codes=codes, asy=asy, equal=[bool(np.array_equal(g, (xA, xB)[i % 2])) for i, g in enumerate(got)])
    for d in park + dEta + [dvB]:
        d.free()

    # ---- a non-positive pivot, then good values on the same context
    order = api.schur_cam_order_host(lam)[0]
    sep = int(np.flatnonzero(np.diff(order) < 0)[-1]) + 1   # (as tests/test_gpu_cam_order.py: the last drop opens the separators)
    where = {"first tile": int(order[3]), "arc B": int(order[sep - 10]), "separator": int(order[sep + 10])}
    dvBad = api.DeviceArray(ctx, lam.vals.size)
    bad = {}
    for tag, cam in where.items():
        dvBad.upload(bad_values(lam, cam))
        dr.upload(eta)
        code = ctx.factor_solve_device(dvBad.ptr, dr.ptr)
        a0 = ctx.info("SOLVE_ASYNC")
        dr.upload(eta)
        code_good = ctx.factor_solve_device(dvA.ptr, dr.ptr)
        x = dr.download()
        bad[tag] = dict(code=code, asy=a0, code_good=code_good, good_equal=bool(np.array_equal(x, xA)),
                        streamed=ctx.info("DENSE_STREAMED"))
    out["bad pivots"] = bad
    for d in (dvBad, dvA, dr):
        d.free()
    ctx.close()

    # ---- two landmark shards on one device: pack, sum on the host (the all-reduce), unpack, finish
    lam, eta = fx73.make_any("edges63")
    ctxs, bufs, asy = [], [], []
    for r in range(2):
        c = context(lam, (r, 2))
        dv, dr = api.DeviceArray.from_host(c, lam.vals), api.DeviceArray.from_host(c, eta)
        dS, dP = api.DeviceArray(c, c.schur_buffer_size()), api.DeviceArray(c, c.schur_packed_size())
        c.schur_form(dv.ptr, dr.ptr, dS.ptr)
        c.schur_pack(dS.ptr, dP.ptr)
        c.synchronize()
        ctxs.append(c)
        bufs.append((dv, dr, dS, dP))
    psum = sum(b[3].download() for b in bufs)
    h = hashlib.sha256()
    for c, (dv, dr, dS, dP) in zip(ctxs, bufs):
        dP.upload(psum)
        c.schur_unpack(dP.ptr, dS.ptr)
        assert c.schur_finish(dv.ptr, dS.ptr, dr.ptr) == 0
        asy.append(c.info("SOLVE_ASYNC"))
        h.update(dr.download().tobytes())   # (the download synchronizes with the finish that returned early)
    out["two shards"] = dict(x=h.hexdigest(), asy=asy)
    for c, b in zip(ctxs, bufs):
        for d in b:
            d.free()
        c.close()

    np.savez(out_path, **arrays)
    return out


if __name__ == "__main__":
    print("RESULT " + json.dumps(run(sys.argv[1], json.loads(sys.argv[2]))))
