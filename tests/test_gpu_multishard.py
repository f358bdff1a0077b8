"""GPU: the multi-GPU split API (spp_set_shard / spp_schur_form / all-reduce / spp_schur_finish) driven
on ONE device: two contexts own the two landmark shards, their partial S | rhs buffers are summed on
the host (standing in for the RCCL all-reduce of bench.py), each context finishes on the summed
buffer. The union of the shards' solutions must equal the unsharded solve.

Further down, on the edge fixtures of tests/schur_fixtures.py and tests/schur_fixtures_73.py (6-, 3- and 7-wide poses):
the merged sharded solution against the longdouble reference of tests/schur_ref.py, the layout of spp_schur_pack against
what include/spp_hip.h states, and a shard that owns no landmark."""
import numpy as np
import pytest

import schur_fixtures_73 as fx73
import schur_ref
from slam_plus_plus_amd import api, synth
from oracle import spp_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,world,mode", [("ba_small", 2, api.MODE_SCHUR), ("ba_interleaved", 3, api.MODE_SCHUR),
                                             ("ba_medium", 2, api.MODE_SCHUR), ("ba_small", 2, api.MODE_SCHUR_SPARSE),
                                             ("ba_banded", 3, api.MODE_SCHUR_SPARSE)])
def test_sharded_schur_equals_unsharded(name, world, mode):
    prob = synth.make(name)
    lam, eta = orc.assemble(prob)
    full = api.CLinearSolver_HIP(mode=mode)
    xfull = eta.copy()
    assert full.Solve_PosDef_Blocky(lam, xfull)
    ctxs, bufs = [], []
    for r in range(world):
        c = api.Context(0)
        c.set_shard(r, world)
        c.analyze(lam, mode)
        assert c.info("MODE") == mode
        dv = api.DeviceArray.from_host(c, lam.vals)
        dr = api.DeviceArray.from_host(c, eta)
        dS = api.DeviceArray(c, c.schur_buffer_size())
        c.schur_form(dv.ptr, dr.ptr, dS.ptr)
        c.synchronize()
        ctxs.append(c)
        bufs.append((dv, dr, dS))
    assert sum(c.info("N_LANDMARKS") for c in ctxs) == int((lam.dim == 3).sum())
    # pack -> sum -> unpack: what bench.py sends through the RCCL all-reduce (upper trapezoid only)
    packed = []
    for c, (dv, dr, dS) in zip(ctxs, bufs):
        dP = api.DeviceArray(c, c.schur_packed_size())
        c.schur_pack(dS.ptr, dP.ptr)
        c.synchronize()
        packed.append(dP)
    if mode == api.MODE_SCHUR:
        nblk = ctxs[0].info("S_LD") // 128
        assert packed[0].n == 128 * 128 * nblk * (nblk + 1) // 2 <= bufs[0][2].n
    else:  # sparse reduced system: block values | rhs, the same structure (union over all landmarks) on every rank
        assert len({c.info("S_NNZB") for c in ctxs}) == 1 and ctxs[0].info("S_NNZB") == full.ctx.info("S_NNZB")
        assert packed[0].n == bufs[0][2].n == 36 * ctxs[0].info("S_NNZB") + ctxs[0].info("N_REDUCED")
    psum = sum(p.download() for p in packed)  # the all-reduce
    for c, (dv, dr, dS), dP in zip(ctxs, bufs, packed):
        dP.upload(psum)
        c.schur_unpack(dP.ptr, dS.ptr)
        c.synchronize()
    total = bufs[0][2].download()
    x = np.zeros_like(eta)
    dl = int(lam.dim.min())
    for r, (c, (dv, dr, dS)) in enumerate(zip(ctxs, bufs)):
        assert c.schur_finish(dv.ptr, dS.ptr, dr.ptr) == 0
        c.synchronize()
        xr = dr.download()
        if r == 0:
            for b in np.flatnonzero(lam.dim != dl):
                x[lam.base[b]:lam.base[b + 1]] = xr[lam.base[b]:lam.base[b + 1]]
        for b in orc.landmark_shard(lam, r, world):
            x[lam.base[b]:lam.base[b + 1]] = xr[lam.base[b]:lam.base[b + 1]]
        # every rank holds the same pose update
        pb = np.flatnonzero(lam.dim != dl)[0]
        assert np.allclose(xr[lam.base[pb]:lam.base[pb + 1]], xfull[lam.base[pb]:lam.base[pb + 1]], rtol=1e-9, atol=0)
    assert np.linalg.norm(x - xfull) / np.linalg.norm(xfull) < 1e-11
    for c, b in zip(ctxs, bufs):
        for d in b:
            d.free()
        c.close()


# ---- the split API against the longdouble reference of tests/schur_ref.py, the packed layout, a shard without landmarks ----
NB = 128
REF_CASES = [("edges63", 3, api.MODE_SCHUR), ("edges32", 2, api.MODE_SCHUR), ("edges73", 2, api.MODE_SCHUR),
             ("edges73_aligned", 3, api.MODE_SCHUR_SPARSE)]
_RUNS = {}


def _sharded_run(name, world, mode):
    """form and pack on every rank; the sums of the full and of the packed buffers (the all-reduce, on the host); then on
    every rank a finish on the summed full buffer, and a finish behind an unpack of the summed packed buffer into a buffer
    full of NaN. Everything downloaded, the contexts closed; run once per case."""
    key = (name, world, mode)
    if key in _RUNS:
        return _RUNS[key]
    lam, eta = fx73.make_any(name)
    ctxs, arrs, full, packed = [], [], [], []
    for r in range(world):
        c = api.Context(0)
        c.set_shard(r, world)
        c.analyze(lam, mode)
        assert c.info("MODE") == mode
        dv, dr = api.DeviceArray.from_host(c, lam.vals), api.DeviceArray.from_host(c, eta)
        dS, dP = api.DeviceArray(c, c.schur_buffer_size()), api.DeviceArray(c, c.schur_packed_size())
        dP.upload(np.full(dP.n, np.nan))   # (the pack must write every entry of the packed buffer)
        c.schur_form(dv.ptr, dr.ptr, dS.ptr)
        c.schur_pack(dS.ptr, dP.ptr)
        c.synchronize()
        full.append(dS.download())
        packed.append(dP.download())
        ctxs.append(c)
        arrs.append((dv, dr, dS, dP))
    fsum, psum = sum(full), sum(packed)
    out = dict(lam=lam, eta=eta, full=full, packed=packed, fsum=fsum, psum=psum, x_full=[], x_unpacked=[], codes=[],
               n_lm=[c.info("N_LANDMARKS") for c in ctxs], ld=ctxs[0].info("S_LD"), n_red=ctxs[0].info("N_REDUCED"),
               nnzb=[c.info("S_NNZB") for c in ctxs])
    for c, (dv, dr, dS, dP) in zip(ctxs, arrs):
        dS.upload(fsum)
        dr.upload(eta)
        out["codes"].append(c.schur_finish(dv.ptr, dS.ptr, dr.ptr))
        out["x_full"].append(dr.download())
        dS.upload(np.full(dS.n, np.nan))
        dP.upload(psum)
        dr.upload(eta)
        c.schur_unpack(dP.ptr, dS.ptr)
        out["codes"].append(c.schur_finish(dv.ptr, dS.ptr, dr.ptr))
        out["x_unpacked"].append(dr.download())
    for c, a in zip(ctxs, arrs):
        for d in a:
            d.free()
        c.close()
    _RUNS[key] = out
    return out


def _merged(run, world):
    """rank 0's poses and every rank's own landmarks (dealt round-robin over the eliminated blocks in ascending order)"""
    lam = run["lam"]
    is_lm = lam.dim == lam.dim.min()
    lms = np.flatnonzero(is_lm)
    x = np.full(lam.n, np.nan)
    for r in range(world):
        mine = np.concatenate([np.flatnonzero(~is_lm)] * (r == 0) + [lms[r::world]]).astype(np.int64)
        idx = schur_ref.pose_index(lam, mine)
        x[idx] = run["x_unpacked"][r][idx]
    return x


@pytest.mark.parametrize("name,world,mode", REF_CASES)
def test_merged_sharded_solution_matches_the_reference(name, world, mode):
    """not the library's own unsharded x: the longdouble reference of the whole system"""
    run = _sharded_run(name, world, mode)
    lam, eta = run["lam"], run["eta"]
    assert run["codes"] == [0] * (2 * world)
    elim = schur_ref.guided_elim(lam)
    assert sum(run["n_lm"]) == elim.size
    R = schur_ref.schur_ref(lam, eta, elim)
    sparse = mode != api.MODE_SCHUR
    # the summed S | rhs (three or two roundings more than one rank's: inside the same bound, which counts every pair)
    rs = schur_ref.check_schur_buffer(R, run["fsum"], sparse, run["ld"])
    rl, rc = schur_ref.check_solution(R, lam, eta, _merged(run, world))
    print("%s world %d mode %d: largest error / bound: summed S | rhs %.3f, landmark part %.3f, pose part %.3f" % (name, world, mode, rs, rl, rc))
    # every rank holds the same pose update: the same buffer, the same factorization
    poses = schur_ref.pose_index(lam, R.poses)
    for r in range(1, world):
        assert np.array_equal(run["x_unpacked"][r][poses], run["x_unpacked"][0][poses]), r


@pytest.mark.parametrize("name,world,mode", REF_CASES)
def test_packed_layout_is_what_the_header_states(name, world, mode):
    """include/spp_hip.h: 128-column panels, rows 0 .. end of the panel's diagonal block, column-major inside the panel,
    128^2 nblk (nblk + 1) / 2 doubles; the sparse buffer travels as it is. The reduced rhs is column n_red of the dense
    buffer: it travels INSIDE the last panel (panel n_red // 128 = nblk - 1, its column n_red % 128, rows 0 .. n_red - 1),
    not behind the panels (spp_schur_pack packs whole panels and nothing else)."""
    run = _sharded_run(name, world, mode)
    n_red = run["n_red"]
    for r in range(world):
        S, P = run["full"][r], run["packed"][r]
        if mode != api.MODE_SCHUR:
            dp = int(run["lam"].dim.max())
            assert P.size == S.size == dp * dp * run["nnzb"][r] + n_red and len(set(run["nnzb"])) == 1
            assert np.array_equal(P, S), "the sparse S | rhs travels as it is"
            continue
        ld = run["ld"]
        nblk = ld // NB
        assert S.size == ld * ld and P.size == NB * NB * nblk * (nblk + 1) // 2
        S2 = S.reshape((ld, ld), order="F")
        want = np.concatenate([S2[:NB * (k + 1), NB * k:NB * (k + 1)].ravel(order="F") for k in range(nblk)])
        assert np.array_equal(P, want), (r, "packed buffer differs from the gather of the header's layout")
        k = n_red // NB
        assert k == nblk - 1, "the rhs column lies in the last panel"
        at = NB * NB * (k * (k + 1) // 2) + (n_red % NB) * NB * (k + 1)
        assert np.array_equal(P[at:at + n_red], S2[:n_red, n_red]) and S2[:n_red, n_red].any(), "where the reduced rhs travels"
        assert not S2[:, n_red + 1:].any() and not S2[n_red:, n_red].any(), "padding columns of a formed buffer are zero"
    # an unpack into a buffer full of NaN, then a finish: the bits of a finish on the summed full buffer -- nothing outside
    # the packed trapezoid is read
    for r in range(world):
        assert np.array_equal(run["x_unpacked"][r], run["x_full"][r]), r
    assert run["codes"] == [0] * (2 * world)


@pytest.mark.parametrize("mode", [api.MODE_SCHUR, api.MODE_SCHUR_SPARSE])
@pytest.mark.parametrize("name", ["tiny_shards", "tiny_shards73"])
def test_a_shard_without_landmarks(name, mode):
    """2 landmarks, 3 shards: rank 2 owns nothing (nl == 0, no == 0 in every launch of the form and the finish)"""
    world = 3
    run = _sharded_run(name, world, mode)
    lam, eta = run["lam"], run["eta"]
    assert run["n_lm"] == [1, 1, 0]
    elim = schur_ref.guided_elim(lam)
    sparse = mode != api.MODE_SCHUR
    ratios = []
    for r in range(world):
        Rr = schur_ref.schur_ref(lam, eta, elim, r, world)
        ratios.append(schur_ref.check_schur_buffer(Rr, run["full"][r], sparse, run["ld"]))
    assert not run["full"][2].any() and not run["packed"][2].any(), "the empty rank's S | rhs is not exact zeros"
    assert run["full"][0].any() and run["full"][1].any()
    R = schur_ref.schur_ref(lam, eta, elim)
    assert R.has_A[1, 2]
    rs = schur_ref.check_schur_buffer(R, run["fsum"], sparse, run["ld"])
    assert run["codes"] == [0] * (2 * world), "spp_schur_finish on every rank"
    poses = schur_ref.pose_index(lam, R.poses)
    for r in range(world):
        assert np.array_equal(run["x_unpacked"][r], run["x_full"][r]), r
        assert np.array_equal(run["x_unpacked"][r][poses], run["x_unpacked"][0][poses]), (r, "pose part")
    rl, rc = schur_ref.check_solution(R, lam, eta, _merged(run, world))
    print("%s mode %d: largest error / bound: per rank %s, sum %.3f, landmark part %.3f, pose part %.3f" % (
        name, mode, ["%.3f" % q for q in ratios], rs, rl, rc))
