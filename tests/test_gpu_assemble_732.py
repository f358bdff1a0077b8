"""The edge shape (7,3,2) -- a projection from a 3-wide point into a 7-wide Sim(3) camera, CEdgeP2C_XYZ_Sim3_G, reference
include/slam/Sim3_Types.h:492-595; the library's vertex order is camera first -- through both assembly entry points: Lambda
and eta against a dense float64 sum of the per-edge terms (tests/rocv_ref.dense_lambda), bound 1e-13 of the largest entry
as in tests/test_gpu_assemble_631.py. The shape lives in plans of one group: every other combination is refused."""
import numpy as np
import pytest

from slam_plus_plus_amd import api
from test_gpu_assemble_unary import _assemble, _binary, _check, _no_plan, E_UNSUPPORTED

pytestmark = pytest.mark.gpu


def _camera_graph(rng):
    """303 cameras (7) and 320 points (3), ids mixed so that the blocks come in both orientations. Camera 0 sees 300 points,
    camera 1 sees 25, camera 2 sees 24, camera 3 ONE; point 0 is seen by 300 cameras (299 of them, twice by camera 4: a block
    fed by two edges); every other vertex has a few edges."""
    nc, npt = 303, 320
    dim = np.array([7] * nc + [3] * npt, dtype=np.int32)[rng.permutation(nc + npt)]
    C, P = np.flatnonzero(dim == 7), np.flatnonzero(dim == 3)
    v0 = np.concatenate([np.full(300, C[0]), np.full(25, C[1]), np.full(24, C[2]), [C[3]], C[4:], [C[4]], C[5:25]])
    v1 = np.concatenate([P[20:320], P[1:26], P[1:25], [P[1]], np.full(nc - 4, P[0]), [P[0]], P[1:21]])
    order = rng.permutation(v0.size)
    v0, v1 = v0[order], v1[order]
    deg = np.bincount(np.concatenate([v0, v1]), minlength=dim.size)
    assert [deg[C[k]] for k in range(4)] == [300, 25, 24, 1] and deg[P[0]] == 300
    assert 0.3 < (v1 < v0).mean() < 0.7, "blocks in both orientations"
    return dim, _binary(rng, dim, v0, v1, 7, 3, 2), C, P


def test_one_group_through_both_entry_points(hip_ctx):
    ctx = hip_ctx
    rng = np.random.default_rng(732)
    dim, g, C, P = _camera_graph(rng)
    for damping, unary in ((0.0, -1), (0.3, int(C[0])), (0.0, int(P[0]))):
        st = _check(ctx, [g], None, unary, damping)            # (two runs inside: the same bits)
        _, [(vals, eta)] = _assemble(ctx, [g], None, unary, damping, repeat=1)
        # spp_assemble_analyze + spp_assemble_device: the same bits
        st1 = ctx.assemble_analyze(dim, g.v0, g.v1, 7, 3, 2, unary)
        arrs = [api.DeviceArray.from_host(ctx, np.ascontiguousarray(g[k]).ravel()) for k in ("J0", "J1", "Om", "r")]
        dv, de = api.DeviceArray(ctx, st1.nvals), api.DeviceArray(ctx, st1.n)
        ctx.assemble_device(*[a.ptr for a in arrs], damping, dv.ptr, de.ptr)
        assert all(np.array_equal(getattr(st, k), getattr(st1, k)) for k in ("col_ptr", "row_idx", "blk_off"))
        assert np.array_equal(dv.download(), vals) and np.array_equal(de.download(), eta)
        for d in arrs + [dv, de]:
            d.free()
    # a position order that is not the edge order
    _check(ctx, [g], [rng.permutation(g.v0.size)])


def test_the_assembled_structure_takes_the_schur_path(hip_ctx):
    """the structure of a (7,3,2) plan is one the Schur stage accepts: widths {7, 3}, landmarks not connected"""
    ctx = hip_ctx
    dim, g, C, P = _camera_graph(np.random.default_rng(733))
    st = ctx.assemble_analyze(dim, g.v0, g.v1, 7, 3, 2, -1)
    ctx.analyze(st, api.MODE_AUTO)
    assert ctx.info("MODE") == api.MODE_SCHUR
    assert ctx.info("N_REDUCED") == 7 * C.size and ctx.info("N_LANDMARKS") == P.size


def test_refused_combinations_leave_no_plan(hip_ctx):
    ctx = hip_ctx
    dim = np.array([7, 3, 7, 3, 6], dtype=np.int32)      # (vertex 4 belongs to the refused (6,3,2) groups alone)
    ok = ([0], [1], 7, 3, 2)

    def refused(groups):
        ctx.assemble_analyze_groups(dim[:4], [ok], None, -1)   # a plan to lose
        assert not _no_plan(ctx)
        with pytest.raises(api.SppError, match="spp error %d" % E_UNSUPPORTED):
            ctx.assemble_analyze_groups(dim, groups, None, -1)
        assert _no_plan(ctx)

    refused([ok, ([2], [3], 7, 3, 2)])                      # the shape twice
    refused([ok, ([4], [3], 6, 3, 2)])                      # beside another binary shape, either order
    refused([([4], [3], 6, 3, 2), ok])
    refused([ok, ([1, 3], None, 3, 0, 3)])                  # beside a group of unary edges
    refused([([1, 3], None, 3, 0, 3), ok])
    for d0, d1, rd in ((7, 3, 3), (7, 3, 1), (7, 7, 7), (3, 7, 2), (7, 2, 2)):   # neighbouring shapes that do not exist
        refused([([0], [1], d0, d1, rd)])
    # the one-group entry point refuses them as well
    ctx.assemble_analyze(dim[:4], [0], [1], 7, 3, 2, -1)
    with pytest.raises(api.SppError, match="spp error %d" % E_UNSUPPORTED):
        ctx.assemble_analyze(dim[:4], [0], [1], 7, 3, 3, -1)
    assert _no_plan(ctx)


def test_robust_weights_are_refused_and_the_plan_stays(hip_ctx):
    ctx = hip_ctx
    rng = np.random.default_rng(734)
    dim, g, C, P = _camera_graph(rng)
    st = ctx.assemble_analyze(dim, g.v0, g.v1, 7, 3, 2, -1)
    dw = api.DeviceArray.from_host(ctx, rng.uniform(0.2, 1.0, size=g.v0.size))
    with pytest.raises(api.SppError, match="spp error %d" % E_UNSUPPORTED):
        ctx.assemble_set_edge_weights(dw.ptr)
    with pytest.raises(api.SppError, match="spp error %d" % E_UNSUPPORTED):
        ctx.assemble_set_group_edge_weights(0, dw.ptr)
    # the plan is still there, and plain: the assembly gives the unweighted sums
    assert not _no_plan(ctx)
    arrs = [api.DeviceArray.from_host(ctx, np.ascontiguousarray(g[k]).ravel()) for k in ("J0", "J1", "Om", "r")]
    dv, de = api.DeviceArray(ctx, st.nvals), api.DeviceArray(ctx, st.n)
    ctx.assemble_device(*[a.ptr for a in arrs], 0.0, dv.ptr, de.ptr)
    _, [(vals, eta)] = _assemble(ctx, [g], None, -1, 0.0, repeat=1)
    assert np.array_equal(dv.download(), vals) and np.array_equal(de.download(), eta)
    for d in arrs + [dv, de, dw]:
        d.free()


@pytest.mark.parametrize("n", [1, 257, 65537])
def test_max_hessian_diagonal_of_the_shape(hip_ctx, n):
    """spp_edge_hessian_maxdiag_device (2,7,3) against numpy: max over edges and both vertices of diag(J^T Omega J). An
    entry is a sum of 4 products of three factors: 2 roundings per product + 3 additions, bound (2 + 3) eps on the sum of
    the terms' magnitudes (at most 4 |Omega|max |J|max^2 -- the planted entry dominates, so its own value is the scale)"""
    rng = np.random.default_rng(735 + n % 7)
    J0, J1 = rng.uniform(-1, 1, size=(n, 7, 2)), rng.uniform(-1, 1, size=(n, 3, 2))   # [e, column, row]: RD x D column-major
    a = rng.normal(size=(n, 2, 2))
    Om = np.einsum("eij,ekj->eik", a, a) / 8 + np.eye(2)
    side = n % 2                                       # the maximum: the last edge, the camera's last column / the point's
    (J0 if side == 0 else J1)[n - 1, -1] = [4.0, -4.0]
    d0 = np.einsum("eci,eij,ecj->ec", J0, Om, J0)
    d1 = np.einsum("eci,eij,ecj->ec", J1, Om, J1)
    ref = float(max(d0.max(), d1.max()))
    assert ref == float((d0 if side == 0 else d1)[n - 1, -1]) and ref >= 16.0
    mag = float(np.einsum("i,ij,j->", [4.0, 4.0], np.abs(Om[n - 1]), [4.0, 4.0]))
    d = [api.DeviceArray.from_host(hip_ctx, np.ascontiguousarray(x).ravel()) for x in (J0, J1, Om)]
    got = hip_ctx.edge_hessian_maxdiag_device(n, 2, 7, 3, d[0].ptr, d[1].ptr, d[2].ptr)
    assert got == hip_ctx.edge_hessian_maxdiag_device(n, 2, 7, 3, d[0].ptr, d[1].ptr, d[2].ptr)
    assert abs(got - ref) <= 2 * 5 * 2.0 ** -52 * mag     # (numpy's own einsum carries the same bound: twice)
    for x in d:
        x.free()
