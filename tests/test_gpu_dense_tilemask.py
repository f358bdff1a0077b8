"""GPU: the streamed dense factor with a tile mask (spp_dense_posv_masked; the Schur stage hands it the filled tile pattern
of S) against the same launch with every tile. A skipped rank-128 update subtracts a product with an all-zero row tile
and a skipped tile is zero before and after, so factor and solution must EQUAL the full-mask run's (numpy.array_equal:
-0 == 0), and repeats must be bit-identical. SPP_TAIL_MASK is read once per process: the Schur stage is compared between
two child processes, as tests/test_gpu_schur_schedules.py does for its switches."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from slam_plus_plus_amd import api

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
NB, BS = 128, 6


def _blocks(kind, nblk):
    I, J = np.triu_indices(nblk)
    w = max(2, nblk // 10)
    if kind == "band":
        keep = J - I <= w
    elif kind == "band+border":
        keep = (J - I <= w) | (J >= nblk - max(3, nblk // 8))
    elif kind == "arrow":
        keep = (I == J) | (J >= nblk - 4)
    elif kind == "blockdiag":       # diagonal blocks of 37 cameras = 222 rows: they straddle the tile edges
        keep = I // 37 == J // 37
    elif kind == "blockdiag64":     # 384 rows = three tiles exactly: every third diagonal tile receives no update at all
        keep = I // 64 == J // 64
    else:
        raise ValueError(kind)
    return I[keep], J[keep]


def _spd(kind, n, seed):
    """an SPD matrix of 6 x 6 blocks on the pattern `kind` (the last block cut at n), its block list and a rhs"""
    nblk = -(-n // BS)
    I, J = _blocks(kind, nblk)
    rng = np.random.default_rng(seed)
    P = np.zeros((nblk, nblk), bool)
    P[I, J] = True
    E = np.kron(P, np.ones((BS, BS), bool))[:n, :n]
    A = np.where(E, rng.standard_normal((n, n)), 0.0)
    A = np.triu(A, 1)
    A = A + A.T
    A[np.diag_indices(n)] = np.abs(A).sum(axis=1) + 1.0 + rng.random(n)
    return A, I, J, rng.standard_normal(n)


def _posv(ctx, A, b, words):
    n = A.shape[0]
    dA = api.DeviceArray.from_host(ctx, np.asfortranarray(A).reshape(-1, order="F"))
    db = api.DeviceArray.from_host(ctx, b)
    w = np.ascontiguousarray(words, dtype=np.uint64)
    st = ctx._check(ctx.lib.spp_dense_posv_masked(ctx.h, dA.ptr, n, n, db.ptr, w.ctypes.data if w.size else None, w.size))
    streamed = ctx.info("DENSE_STREAMED")
    R = np.triu(dA.download().reshape((n, n), order="F"))
    x = db.download()
    dA.free()
    db.free()
    return st, R, x, streamed


CASES = [("band", 300), ("arrow", 385), ("blockdiag", 1000), ("band+border", 1280), ("band", 2560), ("blockdiag", 2700),
         ("band+border", 3333), ("arrow", 3840), ("band+border", 5226), ("band", 5632), ("blockdiag", 5631),
         ("blockdiag64", 2700), ("blockdiag64", 5632)]


@pytest.mark.parametrize("kind,n", CASES)
def test_masked_factor_and_solution_equal_the_full_mask_run(hip_ctx, kind, n):
    A, I, J, b = _spd(kind, n, n)
    Tr = -(-n // NB)
    words, _ = api.tile_mask_host(n, BS, I, J, True, True)
    raw, _ = api.tile_mask_host(n, BS, I, J, True, False)      # not closed: the call closes it
    assert len(words) == Tr
    ntile = sum(bin(int(w)).count("1") for w in words)
    full_tiles = Tr * (n // NB + 1) - Tr * (Tr - 1) // 2
    if kind != "arrow" and Tr > 3:
        assert ntile < full_tiles, "the case does not exercise the mask"
    st0, R0, x0, s0 = _posv(hip_ctx, A, b, [])
    assert st0 == 0 and s0 == Tr, (st0, s0)          # the whole factorization was the streamed launch
    assert np.abs(A @ x0 - b).max() / np.abs(b).max() < 1e-12
    rng = np.random.default_rng(1)
    extra = words.copy()                              # a superset: random extra tiles
    for i in range(Tr):
        extra[i] |= np.uint64(int(rng.integers(0, 1 << 62)) & ~((1 << i) - 1) & ((1 << (n // NB + 1)) - 1))
    for tag, w in (("filled", words), ("filled again", words), ("unfilled", raw), ("superset", extra)):
        st, R, x, s = _posv(hip_ctx, A, b, w)
        assert st == 0 and s == Tr, (tag, st, s)
        assert np.array_equal(R, R0), (tag, "R differs from the full-mask run", int((R != R0).sum()))
        assert np.array_equal(x, x0), (tag, "x differs from the full-mask run")
    # outside the filled pattern the factor is exactly zero (those tiles were never written)
    for i in range(Tr):
        for j in range(i, Tr):
            if not (int(words[i]) >> j) & 1:
                assert not R0[NB * i:NB * (i + 1), NB * j:NB * (j + 1)].any(), (i, j)


@pytest.mark.parametrize("kind,n,bad", [("band+border", 3333, 2000), ("blockdiag", 2700, 2699), ("band", 1280, 0)])
def test_failed_pivot_is_reported_as_without_the_mask(hip_ctx, kind, n, bad):
    A, I, J, b = _spd(kind, n, n + 1)
    A[bad, bad] = -1.0
    words, _ = api.tile_mask_host(n, BS, I, J, True, True)
    st0, _, _, _ = _posv(hip_ctx, A, b, [])
    st1, _, _, _ = _posv(hip_ctx, A, b, words)
    assert st0 == api.SPP_NOT_POSDEF and st1 == st0, (st0, st1)
    # and the context factors the repaired matrix afterwards, masked
    A[bad, bad] = np.abs(A[bad]).sum() + 1.0
    st, R, x, s = _posv(hip_ctx, A, b, words)
    assert st == 0 and np.abs(A @ x - b).max() / np.abs(b).max() < 1e-12


CHILD = r"""
import hashlib, json, sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
from slam_plus_plus_amd import api, synth
from oracle import spp_oracle as orc
import schur_fixtures as fx

def problem(name):
    if name == "ba_ring300":   # 300 cameras on a circle, each point seen inside a window: S is a cyclic band of 15 tile rows
        return orc.assemble(synth.ba_problem(300, 20000, 100000, 300, heavy_tail=True, name=name))
    if name == "ba_small":
        return orc.assemble(synth.make(name))
    return fx.make(name)

out = {}
for name, mode in json.loads(sys.argv[1]):
    lam, eta = problem(name)
    xs = []
    ctx = api.Context(0, 0)
    ctx.analyze(lam, mode)
    dv = api.DeviceArray.from_host(ctx, lam.vals)
    dr = api.DeviceArray(ctx, lam.n)
    for rep in range(2):
        dr.upload(eta)
        assert ctx.factor_solve_device(dv.ptr, dr.ptr) == 0
        xs.append(dr.download())
    assert np.array_equal(xs[0], xs[1]), "%%s: x not bit-reproducible" %% name
    res = np.linalg.norm(lam.matvec(xs[0]) - eta) / np.linalg.norm(eta)
    assert res < 1e-9, (name, res)
    out[name] = dict(x=hashlib.sha256(xs[0].tobytes()).hexdigest(), streamed=ctx.info("DENSE_STREAMED"))
    dv.free(); dr.free(); ctx.close()

# two landmark shards on one device, their S | rhs summed on the host (the all-reduce), each finishing on the sum
for name in json.loads(sys.argv[2]):
    lam, eta = problem(name)
    ctxs, bufs = [], []
    for r in range(2):
        c = api.Context(0, 0)
        c.set_shard(r, 2)
        c.analyze(lam, api.MODE_SCHUR)
        dv = api.DeviceArray.from_host(c, lam.vals)
        dr = api.DeviceArray.from_host(c, eta)
        dS = api.DeviceArray(c, c.schur_buffer_size())
        c.schur_form(dv.ptr, dr.ptr, dS.ptr)
        c.synchronize()
        ctxs.append(c); bufs.append((dv, dr, dS))
    total = sum(b[2].download() for b in bufs)
    h = hashlib.sha256()
    for c, (dv, dr, dS) in zip(ctxs, bufs):
        dS.upload(total)
        assert c.schur_finish(dv.ptr, dS.ptr, dr.ptr) == 0
        c.synchronize()
        h.update(dr.download().tobytes())
    out[name + "/2 shards"] = dict(x=h.hexdigest(), streamed=ctxs[0].info("DENSE_STREAMED"))
    for c, b in zip(ctxs, bufs):
        for d in b:
            d.free()
        c.close()
print("RESULT " + json.dumps(out))
"""

SCHUR_CASES = [("edges63", api.MODE_SCHUR), ("ba_small", api.MODE_SCHUR), ("mis66", api.MODE_SCHUR_MIS),
               ("ba_ring300", api.MODE_SCHUR)]
SHARD_CASES = ["edges63", "ba_ring300"]


def _run(env_extra):
    env = {k: v for k, v in os.environ.items() if k != "SPP_TAIL_MASK"}
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, TESTS), json.dumps(SCHUR_CASES), json.dumps(SHARD_CASES)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "%s: exit %d\n%s%s" % (env_extra, r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def test_schur_stage_gives_the_same_bits_with_and_without_the_mask():
    # the ring problem really has structurally zero tiles (the small fixtures fit in two or three tile rows: full masks)
    from oracle import spp_oracle as orc
    from slam_plus_plus_amd import synth
    lam, _ = orc.assemble(synth.ba_problem(300, 20000, 100000, 300, heavy_tail=True, name="ba_ring300"))
    words = api.schur_tile_mask_host(lam)
    assert len(words) == 15
    assert sum(bin(int(w)).count("1") for w in words) < 15 * 16 // 2
    for rank in range(2):   # a shard's plan carries the mask of the whole structure
        assert np.array_equal(api.schur_tile_mask_host(lam, rank, 2), words)
    masked = _run({"SPP_TAIL_MASK": "1"})
    default = _run({})
    full = _run({"SPP_TAIL_MASK": "0"})
    print({k: v["streamed"] for k, v in masked.items()})
    assert masked["ba_ring300"]["streamed"] == 15 and masked["ba_ring300/2 shards"]["streamed"] == 15
    for k in full:
        assert masked[k]["x"] == full[k]["x"], (k, "x differs between SPP_TAIL_MASK=1 and =0")
        assert default[k]["x"] == masked[k]["x"], (k, "the default is not the masked launch")
