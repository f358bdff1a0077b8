"""GPU: the Schur stage itself (spp_schur.hip, plan in spp_schur_plan.cpp) against the longdouble reference of
tests/schur_ref.py, entry by entry -- not only through the final dx.

spp_schur_form writes S | rhs into a caller buffer: every upper entry must lie within 4 (k_ij + 8 dl) eps M_ij of the
reference (any summation order passes; one dropped block product does not), every other entry of the dense buffer must
be exactly 0.0. Shards (world 2, 3) are checked rank by rank against the reference of their landmarks. The solution is
checked landmark by landmark against C_l^-1 (eta_l - sum B^T x_c) with the library's own pose part x_c, the pose part
against a refined solve of S_ref. The fixtures (tests/schur_fixtures.py) hold split S blocks, A-only blocks, cameras and
landmarks without observations, and a track too long for the fused back-substitution."""
import numpy as np
import pytest

import schur_fixtures as fx
import schur_ref
from slam_plus_plus_amd import api, synth
from oracle import spp_oracle as orc

pytestmark = pytest.mark.gpu

_CACHE = {}


def _problem(name):
    if name not in _CACHE:
        _CACHE[name] = fx.make(name) if name in fx.ALL else orc.assemble(synth.make(name))
    return _CACHE[name]


def _ref(name, lam, eta, elim):
    """the reference of the whole system, kept compact (layouts, bounds, pose solution) for the session"""
    key = (name, tuple(np.asarray(elim).tolist()))
    if key not in _CACHE:
        _CACHE[key] = schur_ref.schur_ref(lam, eta, elim).compact()
    return _CACHE[key]


def _eliminated(ctx, lam):
    n_lm = ctx.info("N_LANDMARKS")
    return np.sort(ctx.ordering(lam.nb)[lam.nb - n_lm:])


def _form(lam, eta, mode, rank=0, world=1):
    """a fresh context: analyze, spp_schur_form into a caller buffer, twice; returns (ctx, buffer, device arrays)"""
    c = api.Context(0)
    if world > 1:
        c.set_shard(rank, world)
    c.analyze(lam, mode)
    dv = api.DeviceArray.from_host(c, lam.vals)
    dr = api.DeviceArray.from_host(c, eta)
    dS = api.DeviceArray(c, c.schur_buffer_size())
    bufs = []
    for _ in range(2):
        dS.upload(np.full(dS.n, np.nan))   # whatever the buffer held: the form must leave nothing of it
        c.schur_form(dv.ptr, dr.ptr, dS.ptr)
        c.synchronize()
        bufs.append(dS.download())
    assert np.array_equal(bufs[0], bufs[1], equal_nan=False), "S | rhs not bit-reproducible"
    return c, bufs[0], (dv, dr, dS)


def _free(c, arrs):
    for d in arrs:
        d.free()
    c.close()


FORM_CASES = [("edges63", api.MODE_SCHUR), ("edges63", api.MODE_SCHUR_SPARSE), ("edges63_long", api.MODE_SCHUR),
              ("edges32", api.MODE_SCHUR), ("edges32", api.MODE_SCHUR_SPARSE), ("ba_small", api.MODE_SCHUR),
              ("lm2d_small", api.MODE_SCHUR_SPARSE), ("mis66", api.MODE_SCHUR_MIS), ("mis33", api.MODE_SCHUR_MIS)]


@pytest.mark.parametrize("name,mode", FORM_CASES)
def test_schur_form_matches_the_reference(name, mode):
    lam, eta = _problem(name)
    c, buf, arrs = _form(lam, eta, mode)
    assert c.info("MODE") == mode
    elim = _eliminated(c, lam)
    if mode != api.MODE_SCHUR_MIS:
        assert np.array_equal(elim, schur_ref.guided_elim(lam))
    R = _ref(name, lam, eta, elim)
    assert c.info("N_REDUCED") == R.n_red and c.info("N_POSES") == R.poses.size
    sparse = mode != api.MODE_SCHUR
    if sparse:
        assert c.info("S_NNZB") == len(R.pattern)
    ratio = schur_ref.check_schur_buffer(R, buf, sparse, c.info("S_LD"))
    print("%s mode %d: largest error / bound of S | rhs %.3f" % (name, mode, ratio))
    if name.startswith("mis"):
        k = R.k[np.triu_indices(R.poses.size)]
        assert k.max() > 2048, "the MIS cut keeps the hubs: their block is split"
    _free(c, arrs)


@pytest.mark.parametrize("name,world,mode", [("edges63", 2, api.MODE_SCHUR), ("edges63", 3, api.MODE_SCHUR_SPARSE),
                                             ("edges63", 3, api.MODE_SCHUR), ("edges32", 2, api.MODE_SCHUR_SPARSE),
                                             ("ba_small", 3, api.MODE_SCHUR_SPARSE)])
def test_shard_partial_schur_matches_the_reference(name, world, mode):
    """each rank's partial S | rhs: its landmarks only, A and eta_P on rank 0 alone; blocks only other ranks' landmarks
    reach are exactly zero (the sparse layout holds the union pattern on every rank)"""
    lam, eta = _problem(name)
    elim = schur_ref.guided_elim(lam)
    ratios = []
    for rank in range(world):
        c, buf, arrs = _form(lam, eta, mode, rank, world)
        R = schur_ref.schur_ref(lam, eta, elim, rank, world)   # (one rank's reference: not kept)
        assert c.info("N_LANDMARKS") == R.lms.size
        ratios.append(schur_ref.check_schur_buffer(R, buf, mode != api.MODE_SCHUR, c.info("S_LD")))
        _free(c, arrs)
    print("%s world %d mode %d: largest error / bound %s" % (name, world, mode, ["%.3f" % r for r in ratios]))


SOLVE_CASES = [("edges63", api.MODE_SCHUR), ("edges63", api.MODE_SCHUR_SPARSE), ("edges63_long", api.MODE_SCHUR),
               ("edges63_long", api.MODE_SCHUR_SPARSE), ("edges32", api.MODE_SCHUR), ("ba_small", api.MODE_SCHUR),
               ("mis66", api.MODE_SCHUR_MIS), ("mis33", api.MODE_SCHUR_MIS)]


@pytest.mark.parametrize("name,mode", SOLVE_CASES)
def test_solution_matches_the_reference(name, mode):
    lam, eta = _problem(name)
    c = api.Context(0)
    c.analyze(lam, mode)
    dv = api.DeviceArray.from_host(c, lam.vals)
    dr = api.DeviceArray(c, lam.n)
    xs = []
    for _ in range(2):
        dr.upload(eta)
        assert c.factor_solve_device(dv.ptr, dr.ptr) == 0
        xs.append(dr.download())
    assert np.array_equal(xs[0], xs[1]), "x not bit-reproducible"
    R = _ref(name, lam, eta, _eliminated(c, lam))
    r_l, r_c = schur_ref.check_solution(R, lam, eta, xs[0])
    print("%s mode %d: landmark part error / bound %.3f, pose part %.3f (cond S %.1e)" % (name, mode, r_l, r_c, R.cond_S))
    _free(c, [dv, dr])


@pytest.mark.parametrize("mode", [api.MODE_SCHUR, api.MODE_SCHUR_SPARSE])
def test_indefinite_landmark_returns_false_and_keeps_eta(mode):
    lam, eta = _problem("ba_small")
    vals = lam.vals.copy()
    lm = int(np.flatnonzero(lam.dim == 3)[17])
    p = lam.col_ptr[lm + 1] - 1
    C = vals[lam.blk_off[p]:lam.blk_off[p] + 9].reshape(3, 3)   # (a view: the shift lands in vals)
    ev = np.linalg.eigvalsh(C)
    C -= 0.5 * (ev[0] + ev[1]) * np.eye(3)   # one negative eigenvalue, two positive ones
    assert np.linalg.eigvalsh(C)[0] < 0 < np.linalg.eigvalsh(C)[-1], "indefinite, not negative definite"
    solver = api.CLinearSolver_HIP(mode=mode)
    x = eta.copy()
    assert solver.Solve_PosDef_Blocky(lam.with_vals(vals), x) is False
    assert np.array_equal(x, eta)
    # and the same solver recovers on the definite system
    assert solver.Solve_PosDef_Blocky(lam, x)
    assert np.linalg.norm(lam.matvec(x) - eta) / np.linalg.norm(eta) < 1e-12
