"""GPU: the Schur stage with 7-wide cameras (Sim(3)) and 3-wide points -- schur_form_t<7, 3> / schur_finish_t<7, 3> --
against the longdouble reference of tests/schur_ref.py, entry by entry, as tests/test_gpu_schur_stage.py does for the
other widths. The block is odd (21 doubles: 8-byte pieces, register-staged fetch), a diagonal block has 49 elements (the
last lane of the reduction owns one element, not two), and 7 does not divide 128: cameras straddle the tiles of the
dense factor (edges73), or fill them exactly (edges73_aligned: the rhs column is the first padding column)."""
import numpy as np
import pytest

import schur_fixtures_73 as fx73
import schur_ref
from slam_plus_plus_amd import api

pytestmark = pytest.mark.gpu

_CACHE = {}


def _problem(name):
    if name not in _CACHE:
        _CACHE[name] = fx73.make(name)
    return _CACHE[name]


def _ref(name, lam, eta, elim):
    key = (name, "ref")
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


NAMES = sorted(fx73.ALL)
MODES = [api.MODE_SCHUR, api.MODE_SCHUR_SPARSE]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_schur_form_matches_the_reference(name, mode):
    lam, eta = _problem(name)
    c, buf, arrs = _form(lam, eta, mode)
    assert c.info("MODE") == mode
    elim = _eliminated(c, lam)
    assert np.array_equal(elim, schur_ref.guided_elim(lam))
    R = _ref(name, lam, eta, elim)
    assert R.dp == 7
    assert c.info("N_REDUCED") == R.n_red and c.info("N_POSES") == R.poses.size
    sparse = mode != api.MODE_SCHUR
    if sparse:
        assert c.info("S_NNZB") == len(R.pattern)
    ratio = schur_ref.check_schur_buffer(R, buf, sparse, c.info("S_LD"))
    print("%s mode %d: largest error / bound of S | rhs %.3f" % (name, mode, ratio))
    _free(c, arrs)


@pytest.mark.parametrize("name,world,mode", [("edges73", 2, api.MODE_SCHUR), ("edges73", 3, api.MODE_SCHUR_SPARSE),
                                             ("edges73_aligned", 2, api.MODE_SCHUR_SPARSE),
                                             ("edges73_aligned", 3, api.MODE_SCHUR)])
def test_shard_partial_schur_matches_the_reference(name, world, mode):
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


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_solution_matches_the_reference(name, mode):
    lam, eta = _problem(name)
    c = api.Context(0)
    c.analyze(lam, mode)
    assert c.info("MODE") == mode
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


def test_auto_picks_the_dense_schur_path():
    lam, eta = _problem("edges73")
    c = api.Context(0)
    c.analyze(lam, api.MODE_AUTO)
    assert c.info("MODE") == api.MODE_SCHUR
    assert c.info("N_REDUCED") == 2240
    c.close()


@pytest.mark.parametrize("mode", MODES)
def test_indefinite_landmark_returns_false_and_keeps_eta(mode):
    lam, eta = _problem("edges73_aligned")
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
