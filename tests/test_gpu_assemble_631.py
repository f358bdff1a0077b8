"""The edge shape (6,3,1) -- ranges from a 6-wide position-velocity vertex to a 3-wide landmark, CEdgePosVel_Landmark3D,
reference include/slam/ROCV_Types.h:77-223 -- through both assembly entry points: Lambda and eta against a dense float64 sum
of the per-edge terms (tests/rocv_ref.dense_lambda), bound 1e-13 of the largest entry as in tests/test_gpu_assemble_groups.py."""
import numpy as np
import pytest

import rocv_ref
from slam_plus_plus_amd import api
from test_gpu_assemble_unary import _assemble, _binary, _check, _no_plan, _unary, E_UNSUPPORTED

pytestmark = pytest.mark.gpu


def _range_graph(rng):
    """303 receivers (6) and 320 transmitters (3), ids mixed so that the blocks come in both orientations. Receiver 0 ranges
    300 transmitters, receiver 1 ranges 25, receiver 2 ranges 24, receiver 3 ONE; transmitter 0 is ranged by 300 receivers
    (299 of them, twice by receiver 4: a block fed by two edges); every other vertex has a few edges."""
    nr, nt = 303, 320
    dim = np.array([6] * nr + [3] * nt, dtype=np.int32)[rng.permutation(nr + nt)]
    R, T = np.flatnonzero(dim == 6), np.flatnonzero(dim == 3)
    v0 = np.concatenate([np.full(300, R[0]), np.full(25, R[1]), np.full(24, R[2]), [R[3]], R[4:], [R[4]], R[5:25]])
    v1 = np.concatenate([T[20:320], T[1:26], T[1:25], [T[1]], np.full(nr - 4, T[0]), [T[0]], T[1:21]])
    order = rng.permutation(v0.size)
    v0, v1 = v0[order], v1[order]
    deg = np.bincount(np.concatenate([v0, v1]), minlength=dim.size)
    assert [deg[R[k]] for k in range(4)] == [300, 25, 24, 1] and deg[T[0]] == 300 and ((v1 < v0).mean() > 0.3)
    return dim, _binary(rng, dim, v0, v1, 6, 3, 1), R, T


def test_one_group_through_both_entry_points(hip_ctx):
    ctx = hip_ctx
    rng = np.random.default_rng(631)
    dim, g, R, T = _range_graph(rng)
    for damping, unary in ((0.0, -1), (0.3, int(R[0])), (0.0, int(T[0]))):
        st = _check(ctx, [g], None, unary, damping)
        _, [(vals, eta)] = _assemble(ctx, [g], None, unary, damping, repeat=1)
        # spp_assemble_analyze + spp_assemble_device: the same bits
        st1 = ctx.assemble_analyze(dim, g.v0, g.v1, 6, 3, 1, unary)
        arrs = [api.DeviceArray.from_host(ctx, np.ascontiguousarray(g[k]).ravel()) for k in ("J0", "J1", "Om", "r")]
        dv, de = api.DeviceArray(ctx, st1.nvals), api.DeviceArray(ctx, st1.n)
        ctx.assemble_device(*[a.ptr for a in arrs], damping, dv.ptr, de.ptr)
        assert all(np.array_equal(getattr(st, k), getattr(st1, k)) for k in ("col_ptr", "row_idx", "blk_off"))
        assert np.array_equal(dv.download(), vals) and np.array_equal(de.download(), eta)
        for d in arrs + [dv, de]:
            d.free()
    # robust weights: the (6,3,1) bodies carry them where every binary shape does
    _check(ctx, [g], None, -1, 0.0, weights=[rng.uniform(0.2, 1.0, size=g.v0.size)])
    # a position order that is not the edge order
    _check(ctx, [g], [rng.permutation(g.v0.size)])


def test_ranges_beside_constant_velocity_edges_and_priors(hip_ctx):
    """the ROCV plan: (6,6,6) + (6,3,1) + unary (3,3), and a unary (6,6) group as the fourth"""
    rng = np.random.default_rng(632)
    dim, g_rng, R, T = _range_graph(rng)
    g_cv = _binary(rng, dim, R[:-1], R[1:], 6, 6, 6)
    g_pri = _unary(rng, dim, np.concatenate([T[:40], T[:2]]), 3, 3)
    g_p6 = _unary(rng, dim, R[[0, 3, 7]], 6, 6)
    groups = [g_cv, g_rng, g_pri, g_p6]
    pos = rng.permutation(sum(len(g.v0) for g in groups))
    cuts = np.cumsum([0] + [len(g.v0) for g in groups])
    seq = [pos[a:b] for a, b in zip(cuts, cuts[1:])]
    _check(hip_ctx, groups, seq)
    _check(hip_ctx, groups[:3], None, unary_vertex=int(T[0]), damping=0.1)


def test_two_shapes_of_the_widths_6_3_in_one_plan_are_rejected(hip_ctx):
    ctx = hip_ctx
    dim = np.array([6, 3, 6, 3], dtype=np.int32)
    for rd in (2, 3):
        for groups in ([([0], [1], 6, 3, 1), ([2], [3], 6, 3, rd)], [([0], [1], 6, 3, rd), ([2], [3], 6, 3, 1)]):
            ctx.assemble_analyze_groups(dim, [([0], [1], 6, 3, 1)], None, -1)   # a plan to lose
            with pytest.raises(api.SppError, match="spp error %d" % E_UNSUPPORTED):
                ctx.assemble_analyze_groups(dim, groups, None, -1)
            assert _no_plan(ctx)
    ctx.assemble_analyze_groups(dim, [([0], [1], 6, 3, 1), ([2], [3], 6, 3, 1)], None, -1)     # one shape twice is fine
    assert not _no_plan(ctx)


@pytest.mark.parametrize("n", [1, 257, 65537])
def test_max_hessian_diagonal_of_the_range_shape(hip_ctx, n):
    """spp_edge_hessian_maxdiag_device (1,6,3): max over edges and both vertices of diag(J^T Omega J) = Omega J_c^2; one
    product chain of 3 roundings"""
    rng = np.random.default_rng(633 + n % 7)
    J0, J1, Om = rng.uniform(-1, 1, size=(n, 6)), rng.uniform(-1, 1, size=(n, 3)), rng.uniform(0.5, 2.0, size=n)
    J1[n - 1, 1] = 3.0                                            # the maximum: the last edge, the landmark side
    ref = float(Om[n - 1]) * 9.0
    rest = max(float((Om[:, None] * J0 * J0).max()), float((np.delete(Om, n - 1)[:, None] * np.delete(J1, n - 1, axis=0) ** 2).max(initial=0.0)))
    assert rest <= 2.0 < 4.5 <= ref                                  # the planted entry IS the maximum, by far
    d = [api.DeviceArray.from_host(hip_ctx, a.ravel()) for a in (J0, J1, Om)]
    got = hip_ctx.edge_hessian_maxdiag_device(n, 1, 6, 3, d[0].ptr, d[1].ptr, d[2].ptr)
    assert got == hip_ctx.edge_hessian_maxdiag_device(n, 1, 6, 3, d[0].ptr, d[1].ptr, d[2].ptr)
    assert abs(got - ref) <= 3 * 2.0 ** -52 * ref
    for a in d:
        a.free()
