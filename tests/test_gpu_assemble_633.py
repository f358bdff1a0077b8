"""The (6,3,3) edge shape of the device assembly -- XYZ observations of 3-wide landmarks from 6-wide poses -- alone
(spp_assemble_analyze / spp_assemble_device) and beside (6,6,6) odometry (spp_assemble_analyze_groups /
spp_assemble_groups_device), against a dense float64 Lambda built edge by edge in numpy; bound 1e-13 of the largest
entry, the project's bound for an assembled Lambda."""
import functools

import numpy as np
import pytest

from slam_plus_plus_amd import api, synth
from slam_plus_plus_amd.formats import slam3d_linearize
from test_gpu_assemble_groups import _dense, _group_of, _groups, _one_group, _same_structure, _expect_no_plan, \
    BADARG, UNSUPPORTED

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _fixture(name):
    p = synth.make(name)
    return p, slam3d_linearize(p.dim, p.state, p.odo, p.odo_info, p.obs, p.obs_info)


def _close(vals, eta, lam, eta_ref, what):
    dv, de = np.abs(vals - lam.vals).max(), np.abs(eta - eta_ref).max()
    print(what, "max|dLambda| %.3e (max|Lambda| %.3e), max|deta| %.3e (max|eta| %.3e)" % (
        dv, np.abs(lam.vals).max(), de, np.abs(eta_ref).max()))
    assert dv <= 1e-13 * np.abs(lam.vals).max() and de <= 1e-13 * np.abs(eta_ref).max(), what


def test_one_group_633_matches_a_dense_float64_lambda(hip_ctx):
    prob = synth.make("lm3d_small")
    g = _group_of(prob)
    lam, eta = _dense(prob.dim, [g], prob.damping, prob.unary_vertex)
    st, vals, e = _one_group(hip_ctx, prob, prob.damping, prob.unary_vertex)
    assert _same_structure(st, lam)
    _close(vals, e, lam, eta, "lm3d_small")
    # spp_assemble_groups_device on the one-group plan: the same kernels, the same bits; and run to run
    st1, (a, b) = _groups(hip_ctx, prob.dim, [g], None, prob.damping, prob.unary_vertex, repeat=2)
    assert _same_structure(st, st1)
    assert np.array_equal(a[0], vals) and np.array_equal(a[1], e) and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("name", ["slam3d_small", "slam3d_interleaved"])
def test_odometry_and_observations_match_a_dense_float64_lambda(hip_ctx, name):
    p, groups = _fixture(name)
    groups = [_group_of(g) for g in groups]
    if name == "slam3d_interleaved":   # both wave kernels run (degree > 24 in both widths), transposed and plain blocks
        deg = np.bincount(np.concatenate([np.concatenate([g.v0, g.v1]) for g in groups]), minlength=p.dim.size)
        assert (deg[p.dim == 6] > 24).sum() > 0 and (deg[p.dim == 3] > 24).sum() > 0          # n_wave > 0 for 6 and for 3
        assert (deg[p.dim == 6] <= 24).sum() > 0 and (deg[p.dim == 3] <= 24).sum() > 0        # and n_seq
        assert (groups[1].v1 < groups[1].v0).any() and (groups[1].v1 > groups[1].v0).any()
    seq = [p.odo_seq, p.obs_seq]
    lam, eta = _dense(p.dim, groups, 0.0, p.unary_vertex)
    st, (a, b) = _groups(hip_ctx, p.dim, groups, seq, 0.0, p.unary_vertex, repeat=2)
    assert _same_structure(st, lam)
    _close(a[0], a[1], lam, eta, name)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])                           # run to run


def test_633_split_in_two_groups_keeps_the_bits(hip_ctx):
    """even and odd observations as two (6,3,3) groups, h_seq = the original index: every destination sums in the original
    order, also through both wave kernels (the interleaved fixture), so the one-group bits come back"""
    p, (_, prob) = _fixture("slam3d_interleaved")
    ne = prob.v0.size
    even, odd = np.arange(0, ne, 2), np.arange(1, ne, 2)
    st0, v0, e0 = _one_group(hip_ctx, prob, 0.125, prob.unary_vertex)
    st1, v1, e1 = _groups(hip_ctx, prob.dim, [_group_of(prob, even), _group_of(prob, odd)], [even, odd], 0.125, prob.unary_vertex)
    assert _same_structure(st0, st1) and np.array_equal(v0, v1) and np.array_equal(e0, e1)


def test_robust_weights_on_the_633_group(hip_ctx):
    """first / second vertex convention of BaseTypes_Binary.h:768-848: H00, H01, H11 and g1 carry w once, g0 twice"""
    p, groups = _fixture("slam3d_interleaved")
    groups = [_group_of(g) for g in groups]
    w = np.random.default_rng(8).uniform(0.2, 1.0, size=groups[1].v0.size)
    lam, eta = _dense(p.dim, groups, 1e-2, p.unary_vertex, [None, w])
    _, vals, e = _groups(hip_ctx, p.dim, groups, [p.odo_seq, p.obs_seq], 1e-2, p.unary_vertex, [None, w])
    _close(vals, e, lam, eta, "two groups, observations weighted")
    prob = synth.make("lm3d_small")
    w1 = np.random.default_rng(9).uniform(0.2, 1.0, size=prob.v0.size)
    lam, eta = _dense(prob.dim, [_group_of(prob)], prob.damping, prob.unary_vertex, [w1])
    _, vals, e = _one_group(hip_ctx, prob, prob.damping, prob.unary_vertex, weights=w1)
    _close(vals, e, lam, eta, "one group weighted")


def test_lm_scalars_accept_the_633_group(hip_ctx):
    prob = synth.make("lm3d_small")
    ne = prob.v0.size
    up = lambda a: api.DeviceArray.from_host(hip_ctx, np.ascontiguousarray(a).ravel())
    dJ0, dJ1, dOm, dr = up(prob.J0), up(prob.J1), up(prob.Om), up(prob.r)
    Om = prob.Om.reshape(ne, 3, 3)
    chi2 = float(np.einsum("ei,eij,ej->", prob.r, Om, prob.r))
    assert abs(hip_ctx.edge_chi2_device(ne, 3, dr.ptr, dOm.ptr) - chi2) <= 1e-13 * chi2
    J0, J1 = prob.J0.reshape(ne, 6, 3).transpose(0, 2, 1), prob.J1.reshape(ne, 3, 3).transpose(0, 2, 1)
    md = max(np.einsum("eki,ekl,eli->ei", J, Om, J).max() for J in (J0, J1))
    assert abs(hip_ctx.edge_hessian_maxdiag_device(ne, 3, 6, 3, dJ0.ptr, dJ1.ptr, dOm.ptr) - md) <= 1e-13 * md
    scale = float(np.median(np.linalg.norm(prob.r, axis=1)))
    dw = api.DeviceArray(hip_ctx, ne)
    hip_ctx.edge_robust_weights_device(ne, 3, dr.ptr, dw.ptr, scale)
    x = np.sqrt((prob.r ** 2).sum(axis=1)) / scale
    want = np.where(x <= 1.345, 1.0, 1.345 / np.maximum(x, 1.345))    # (a landmark's first observation has r = 0)
    assert (want < 1).any() and (want == 1).any() and np.abs(dw.download() - want).max() <= 1e-13
    for d in (dJ0, dJ1, dOm, dr, dw):
        d.free()


def test_error_codes_of_the_new_shape():
    ctx = api.Context(0)
    dim = np.array([6, 6, 3, 6, 3], dtype=np.int32)
    dim2 = np.array([6, 6, 3, 6, 3, 2], dtype=np.int32)                      # the same graph + a 2-wide vertex
    odo = (np.array([0, 1]), np.array([1, 3]), 6, 6, 6)
    xyz = (np.array([0, 3, 1]), np.array([2, 4, 2]), 6, 3, 3)
    proj = (np.array([0, 3]), np.array([4, 2]), 6, 3, 2)

    def good():
        ctx.assemble_analyze_groups(dim, [odo, xyz], None, 0)
        assert ctx.info("NNZB") > 0

    def rejected(code, groups, dim=dim):
        good()
        with pytest.raises(api.SppError, match=code):
            ctx.assemble_analyze_groups(dim, groups, None, 0)
        _expect_no_plan(ctx)

    rejected(UNSUPPORTED, [proj, xyz])                                       # (6,3,2) beside (6,3,3): one block, two shapes
    rejected(UNSUPPORTED, [odo, xyz, proj])
    rejected(UNSUPPORTED, [odo, (xyz[0], xyz[1], 3, 2, 3)])                  # (3,2,3) stays unsupported
    rejected(BADARG, [odo, (np.array([0, 3, 1]), np.array([2, 5, 2]), 6, 3, 3)], dim2)   # a 2-wide vertex in a (6,3,3) group
    good()
    with pytest.raises(api.SppError, match=BADARG):                          # the one-group entry alike
        ctx.assemble_analyze(dim2, np.array([0, 3]), np.array([2, 5]), 6, 3, 3, 0)
    _expect_no_plan(ctx)
    ctx.assemble_analyze_groups(dim, [odo, proj], None, 0)                   # each of the two beside (6,6,6) is fine
    good()
    ctx.close()
