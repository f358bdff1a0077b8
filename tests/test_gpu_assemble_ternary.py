"""spp_assemble_analyze_ternary / spp_assemble_ternary_device: Lambda and eta of ternary edges (camera 6, point 3,
intrinsics 6 wide with one inert coordinate) from random J / Omega (SPD) / r, no geometry involved, against a longdouble
J^T Omega J reference block by block.

The bound per entry is (2 rd + 2 + depth) eps sum |J|^T |Omega| |J| (eta: sum |J|^T |Omega| |r|), rd = 2; on a diagonal
entry the unary 1.0 and the damping join the sum of magnitudes (they are added to it, each with one rounding: the "+ 2").
depth = the additions a term can pass through, from the kernels (spp_assemble.hip, spp_assemble3.hip), by the number of edges
deg of the destination:
    off-diagonal block of the (camera, point) part      one thread, edge order                    deg - 1
    diagonal block / eta of a camera or point           deg <= 24: one thread                     deg - 1
                                                        else one wave: lanes stride by 64, xor butterfly
                                                                                                  ceil(deg / 64) - 1 + 6
    border destination (touches an intrinsics vertex)   deg <= 24: one thread                     deg - 1
                                                        else chunks of C = ASM_HUB_CHUNK edges: 256 threads stride the chunk
                                                        (C / 256 - 1), butterfly (6), 4 waves in order (3), partials in
                                                        ascending order (chunks - 1)              C / 256 + 8 + ceil(deg / C) - 1
"""
import ctypes
import functools

import numpy as np
import pytest

from slam_plus_plus_amd import api
from slam_plus_plus_amd.blockcsc import structure_from_pairs
from bai_cases import EPS, fixture

pytestmark = pytest.mark.gpu
RD = 2
LD = np.longdouble


@functools.lru_cache(maxsize=None)
def hub_chunk():
    ctx = api.Context(0)
    c = ctx.info("ASM_HUB_CHUNK")
    ctx.close()
    return c


def depth_of(deg, kind):
    """kind: 'ob' off-diagonal block of the binary part, 'v' diagonal block / eta of a camera or point, 'border'"""
    C = hub_chunk()
    if kind == "ob" or deg <= 24:
        return deg - 1
    if kind == "v":
        return -(-deg // 64) - 1 + 6
    return C // 256 + 8 + (-(-deg // C)) - 1


def random_inputs(ne, seed):
    rng = np.random.default_rng(seed)
    J0, J1, J2 = rng.normal(size=(ne, 12)), rng.normal(size=(ne, 6)), rng.normal(size=(ne, 12))
    J2[:, 10:] = 0.0                                   # the inert column
    A = rng.normal(size=(ne, 2, 2))
    Om = np.einsum("eij,ekj->eik", A, A) + 0.5 * np.eye(2)
    return J0, J1, J2, np.ascontiguousarray(Om).reshape(ne, 4), rng.normal(size=(ne, 2))


def reference(dim, v, J, Om, r, unary, damping):
    """longdouble blocks: {(va, vb) role-ordered vertex pair: (value, magnitude sum, degree)} for the six role pairs, and per
    vertex (eta, magnitude, degree); roles 0 camera, 1 point, 2 intrinsics"""
    ne = v[0].size
    nv = dim.size
    Jm = [np.asarray(J[k], dtype=LD).reshape(ne, -1, 2).transpose(0, 2, 1) for k in range(3)]
    Omm, rr = np.asarray(Om, dtype=LD).reshape(ne, 2, 2), np.asarray(r, dtype=LD)
    blocks = {}
    for a in range(3):
        for b in range(a, 3):
            H = np.einsum("eli,elm,emj->eij", Jm[a], Omm, Jm[b])
            S = np.einsum("eli,elm,emj->eij", np.abs(Jm[a]), np.abs(Omm), np.abs(Jm[b]))
            uniq, inv, cnt = np.unique(v[a] * nv + v[b], return_inverse=True, return_counts=True)
            accH, accS = np.zeros((uniq.size,) + H.shape[1:], dtype=LD), np.zeros((uniq.size,) + H.shape[1:], dtype=LD)
            np.add.at(accH, inv, H)
            np.add.at(accS, inv, S)
            for k, key in enumerate(uniq):
                blocks[(int(key // nv), int(key % nv))] = (accH[k], accS[k], int(cnt[k]), (a, b))
    eta = {}
    for a in range(3):
        g = np.einsum("eli,elm,em->ei", Jm[a], Omm, rr)
        S = np.einsum("eli,elm,em->ei", np.abs(Jm[a]), np.abs(Omm), np.abs(rr))
        uniq, inv, cnt = np.unique(v[a], return_inverse=True, return_counts=True)
        accg, accS = np.zeros((uniq.size, g.shape[1]), dtype=LD), np.zeros((uniq.size, g.shape[1]), dtype=LD)
        np.add.at(accg, inv, g)
        np.add.at(accS, inv, S)
        for k, key in enumerate(uniq):
            eta[int(key)] = (accg[k], accS[k], int(cnt[k]), a)
    return blocks, eta


def get_block(st, vals, i, j):
    """block (i, j), i <= j, of the structure as a (dim i, dim j) array"""
    p0, p1 = st.col_ptr[j], st.col_ptr[j + 1]
    p = p0 + int(np.searchsorted(st.row_idx[p0:p1 - 1], i)) if i != j else p1 - 1
    assert st.row_idx[p] == i
    di, dj = int(st.dim[i]), int(st.dim[j])
    return vals[st.blk_off[p]:st.blk_off[p] + di * dj].reshape(dj, di).T


def run_ternary(ctx, dim, v, J, Om, r, unary, damping):
    st = ctx.assemble_analyze_ternary(dim, v[0], v[1], v[2], unary)
    up = lambda a: api.DeviceArray.from_host(ctx, np.ascontiguousarray(a).ravel())
    d = [up(a) for a in (J[0], J[1], J[2], Om, r)]
    dv, de = api.DeviceArray(ctx, st.nvals), api.DeviceArray(ctx, st.n)
    dv.upload(np.full(st.nvals, np.nan))               # every value must be written
    de.upload(np.full(st.n, np.nan))
    ctx.assemble_ternary_device(*[x.ptr for x in d], damping, dv.ptr, de.ptr)
    ctx.synchronize()
    return st, dv.download(), de.download()


def check_against_reference(st, vals, eta, dim, v, J, Om, r, unary, damping):
    """every block and eta segment within the bound; the union pattern; the inert coordinate. Returns the worst quotient
    error / bound."""
    nv = dim.size
    rows = np.concatenate([np.minimum(v[a], v[b]) for a, b in ((0, 1), (0, 2), (1, 2))])
    cols = np.concatenate([np.maximum(v[a], v[b]) for a, b in ((0, 1), (0, 2), (1, 2))])
    want, _, _ = structure_from_pairs(dim, rows, cols)
    assert np.array_equal(st.col_ptr, want.col_ptr) and np.array_equal(st.row_idx, want.row_idx)
    assert np.array_equal(st.blk_off, want.blk_off) and st.nvals == want.nvals
    assert np.isfinite(vals).all() and np.isfinite(eta).all()
    blocks, etas = reference(dim, v, J, Om, r, unary, damping)
    is_intr = np.zeros(nv, dtype=bool)
    is_intr[v[2]] = True
    worst = 0.0
    for (va, vb), (H, S, deg, (a, b)) in blocks.items():
        border = a == 2 or b == 2
        if va == vb:
            S = S.copy()
            H = H.copy()
            live = 5 if is_intr[va] else int(dim[va])
            idx = np.arange(int(dim[va]))
            H[idx, idx] += damping
            S[idx, idx] += damping
            if va == unary:
                H[idx[:live], idx[:live]] += 1
                S[idx[:live], idx[:live]] += 1
            if is_intr[va]:
                H[5, 5] += 1
                S[5, 5] += 1
            kind = "border" if border else "v"
            got = get_block(st, vals, va, va)
            assert np.array_equal(got, got.T)
        else:
            kind = "border" if border else "ob"
            got = get_block(st, vals, va, vb) if va < vb else get_block(st, vals, vb, va).T
        bound = (2 * RD + 2 + depth_of(deg, kind)) * EPS * S
        err = np.abs(np.asarray(got, dtype=LD) - H)
        assert (err <= bound).all(), ((va, vb), deg, kind, float((err / np.maximum(bound, LD(1e-300))).max()))
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
    base = st.base
    for va, (g, S, deg, a) in etas.items():
        bound = (2 * RD + 2 + depth_of(deg, "border" if a == 2 else "v")) * EPS * S
        err = np.abs(np.asarray(eta[base[va]:base[va + 1]], dtype=LD) - g)
        assert (err <= bound).all(), (va, deg, a)
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
    for u in np.flatnonzero(is_intr):                  # the inert coordinate
        D = get_block(st, vals, u, u)
        assert D[5, 5] == 1.0 + damping and not D[5, :5].any() and not D[:5, 5].any() and eta[base[u] + 5] == 0.0
        p0, p1 = st.col_ptr[u], st.col_ptr[u + 1] - 1
        for p in range(p0, p1):                        # blocks above it: its column
            i = int(st.row_idx[p])
            assert not get_block(st, vals, i, u)[:, 5].any()
        for j in range(u + 1, nv):                     # blocks right of it: its row
            p0, p1 = st.col_ptr[j], st.col_ptr[j + 1] - 1
            q = p0 + int(np.searchsorted(st.row_idx[p0:p1], u))
            if q < p1 and st.row_idx[q] == u:
                assert not get_block(st, vals, u, j)[5, :].any()
    return worst


@pytest.mark.parametrize("name", ["bai_tiny", "bai_small"])
@pytest.mark.parametrize("layout", ["first", "last", "interleaved"])
def test_lambda_and_eta_against_longdouble(name, layout):
    """(a) the fixtures' structures with the intrinsics ids first, last and interleaved; the unary factor on vertex 0
    (an intrinsics vertex, a camera, or whatever the shuffle put there)"""
    p = fixture(name, layout)
    v = [np.asarray(p.v0, dtype=np.int64), np.asarray(p.v1, dtype=np.int64), np.asarray(p.v2, dtype=np.int64)]
    J0, J1, J2, Om, r = random_inputs(v[0].size, 5)
    ctx = api.Context(0)
    st, vals, eta = run_ternary(ctx, p.dim, v, (J0, J1, J2), Om, r, 0, 0.375)
    worst = check_against_reference(st, vals, eta, p.dim, v, (J0, J1, J2), Om, r, 0, 0.375)
    print(name, layout, "worst error / bound: %.3f" % worst)
    # a ternary plan is not assembled by the binary entry point: SPP_E_STATE, checked before any pointer is used
    assert ctx.lib.spp_assemble_device(ctx.h, 1, 1, 1, 1, ctypes.c_double(0.0), 1, 1) == -5
    ctx.close()


def _degree_graph():
    """3 cameras of degree 25, 300 and 10 over 300 points, 2 intrinsics vertices (cameras 0, 2 -> the first, camera 1 ->
    the second, so points share both); ids: intrinsics in the middle"""
    cam = np.concatenate([np.zeros(25), np.ones(300), np.full(10, 2)]).astype(np.int64)
    pt = np.concatenate([np.arange(25), np.arange(300), np.arange(290, 300)]).astype(np.int64)
    order = np.random.default_rng(3).permutation(cam.size)
    cam, pt = cam[order], pt[order]
    nv = 3 + 2 + 300
    dim = np.array([6, 6, 6, 6, 6] + [3] * 300, dtype=np.int32)
    cam_id, intr_id = np.array([0, 1, 4]), np.array([2, 3])
    v = [cam_id[cam], 5 + pt, intr_id[cam % 2]]
    return dim, v


def test_the_camera_point_part_is_the_binary_assembly_bit_for_bit():
    """(b) every block and eta segment that touches no intrinsics vertex equals spp_assemble_device on the (6, 3, 2) group
    with the same J0, J1, Omega, r (no unary factor, same damping) bit for bit: cameras of degree 25 and 300 cross the
    sequential and the wave kernel; everything also within the bound"""
    dim, v = _degree_graph()
    J0, J1, J2, Om, r = random_inputs(v[0].size, 6)
    ctx = api.Context(0)
    st, vals, eta = run_ternary(ctx, dim, v, (J0, J1, J2), Om, r, -1, 0.25)
    check_against_reference(st, vals, eta, dim, v, (J0, J1, J2), Om, r, -1, 0.25)
    sb = ctx.assemble_analyze(dim, v[0], v[1], 6, 3, 2, -1)
    up = lambda a: api.DeviceArray.from_host(ctx, np.ascontiguousarray(a).ravel())
    dv, de = api.DeviceArray(ctx, sb.nvals), api.DeviceArray(ctx, sb.n)
    ctx.assemble_device(up(J0).ptr, up(J1).ptr, up(Om).ptr, up(r).ptr, 0.25, dv.ptr, de.ptr)
    ctx.synchronize()
    bvals, beta = dv.download(), de.download()
    ctx.close()
    is_intr = np.zeros(dim.size, dtype=bool)
    is_intr[v[2]] = True
    n_cmp = 0
    for j in range(dim.size):
        if is_intr[j]:
            continue
        assert np.array_equal(eta[st.base[j]:st.base[j + 1]], beta[sb.base[j]:sb.base[j + 1]])
        for p in range(sb.col_ptr[j], sb.col_ptr[j + 1]):
            i = int(sb.row_idx[p])
            assert not is_intr[i]
            assert np.array_equal(get_block(st, vals, i, j), get_block(sb, bvals, i, j)), (i, j)
            n_cmp += 1
    assert n_cmp == 303 + np.unique(v[0] * dim.size + v[1]).size
    deg = np.bincount(v[0])
    assert sorted(deg[deg > 0].tolist()) == [10, 25, 300]


@pytest.mark.parametrize("which", range(7))
def test_hub_degrees(which):
    """(c) one camera, one intrinsics vertex, deg points, deg = 1, 24, 25, C - 1, C, C + 1, 3 C + 5: H02, H22 and g2 cross
    from the sequential kernel to one chunk, to a full chunk, to several; two runs give the same bits"""
    C = hub_chunk()
    deg = [1, 24, 25, C - 1, C, C + 1, 3 * C + 5][which]
    dim = np.array([6, 6] + [3] * deg, dtype=np.int32)
    v = [np.full(deg, 1, dtype=np.int64), 2 + np.arange(deg, dtype=np.int64), np.zeros(deg, dtype=np.int64)]
    J0, J1, J2, Om, r = random_inputs(deg, 7 + which)
    ctx = api.Context(0)
    st, vals, eta = run_ternary(ctx, dim, v, (J0, J1, J2), Om, r, 0, 0.125)
    _, vals2, eta2 = run_ternary(ctx, dim, v, (J0, J1, J2), Om, r, 0, 0.125)
    ctx.close()
    assert np.array_equal(vals, vals2) and np.array_equal(eta, eta2)
    worst = check_against_reference(st, vals, eta, dim, v, (J0, J1, J2), Om, r, 0, 0.125)
    print("degree %d: worst error / bound %.3f" % (deg, worst))


def test_two_intrinsics_vertices_share_points():
    """(d) two cameras with an intrinsics vertex each see the same 30 points (30 > 24 edges: their H02, H22 and g2 take the
    hub reduction), a third camera shares the first one's intrinsics: every point has two (point, intrinsics) blocks, 5 of
    them fed by two edges"""
    pts = np.arange(30, dtype=np.int64)
    cam = np.concatenate([np.zeros(30), np.ones(30), np.full(5, 2)]).astype(np.int64)
    pt = np.concatenate([pts, pts, pts[:5]])
    dim = np.array([3] * 30 + [6] * 5, dtype=np.int32)
    v = [30 + cam, pt, 33 + (cam % 2)]
    J0, J1, J2, Om, r = random_inputs(cam.size, 8)
    ctx = api.Context(0)
    st, vals, eta = run_ternary(ctx, dim, v, (J0, J1, J2), Om, r, 33, 0.5)
    ctx.close()
    check_against_reference(st, vals, eta, dim, v, (J0, J1, J2), Om, r, 33, 0.5)
    for j in (33, 34):
        assert np.array_equal(st.row_idx[st.col_ptr[j]:st.col_ptr[j] + 30], pts)


def test_analysing_the_same_graph_again_keeps_the_solver_plan():
    """the ctx is judged by the UNION structure: the same ternary graph analysed again leaves the solver's symbolic analysis
    in place (spp_get_info MODE still answers), another graph drops it (SPP_E_STATE, -5)"""
    p = fixture("bai_small")
    v = [np.asarray(a, dtype=np.int64) for a in (p.v0, p.v1, p.v2)]
    ctx = api.Context(0)
    st = ctx.assemble_analyze_ternary(p.dim, *v, 0)
    out = ctypes.c_int64()
    assert ctx.lib.spp_get_info(ctx.h, api.INFO["MODE"], ctypes.byref(out)) == -5      # not analysed yet
    ctx.analyze(st, api.MODE_AUTO)
    assert ctx.info("MODE") == api.MODE_SCHUR
    st2 = ctx.assemble_analyze_ternary(p.dim, *v, 0)
    assert np.array_equal(st2.row_idx, st.row_idx) and ctx.info("MODE") == api.MODE_SCHUR and ctx.info("NVALS") == st.nvals
    # a rejected call leaves the solver's plan and the sizes alone as well (and no assembly plan)
    bad = v[2].copy()
    bad[0] = v[0][0]
    assert ctx.lib.spp_assemble_analyze_ternary(ctx.h, p.dim.size, p.dim.ctypes.data, v[0].size, v[0].ctypes.data, v[1].ctypes.data,
                                                bad.ctypes.data, 6, 3, 6, 5, 2, 0) == -1
    assert ctx.info("MODE") == api.MODE_SCHUR and ctx.info("NVALS") == st.nvals
    q = fixture("bai_tiny")
    ctx.assemble_analyze_ternary(q.dim, q.v0, q.v1, q.v2, 0)
    assert ctx.lib.spp_get_info(ctx.h, api.INFO["MODE"], ctypes.byref(out)) == -5
    ctx.close()


def test_error_codes():
    """(e) a shape that is not instantiated: SPP_E_UNSUPPORTED (-6); v0 == v2 or a width mismatch: SPP_E_BADARG (-1), and
    the ctx then holds no plan: spp_assemble_ternary_device gives SPP_E_STATE (-5)"""
    ctx = api.Context(0)
    lib, h = ctx.lib, ctx.h
    dim = np.array([6, 6, 3, 3], dtype=np.int32)
    arr = lambda *a: np.array(a, dtype=np.int64)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def analyze(dim, v0, v1, v2, shape=(6, 3, 6, 2), live2=5, unary=-1):
        return lib.spp_assemble_analyze_ternary(h, dim.size, ptr(dim), v0.size, ptr(v0), ptr(v1), ptr(v2), shape[0], shape[1],
                                                shape[2], live2, shape[3], unary)

    def run():
        return lib.spp_assemble_ternary_device(h, 1, 1, 1, 1, 1, ctypes.c_double(0.0), 1, 1)

    good = (arr(0, 0), arr(2, 3), arr(1, 1))
    assert run() == -5                                              # no plan yet
    assert analyze(dim, *good) == 0
    for shape, live2 in (((6, 3, 5, 2), 5), ((6, 3, 6, 3), 5), ((6, 3, 6, 2), 6), ((3, 3, 6, 2), 5)):
        assert analyze(dim, *good, shape=shape, live2=live2) == -6, shape
        assert run() == -5
    assert analyze(dim, *good) == 0
    assert analyze(dim, arr(0, 1), arr(2, 3), arr(1, 1)) == -1      # v0 == v2 in the second edge
    assert run() == -5
    assert analyze(dim, *good) == 0
    assert analyze(dim, arr(0, 0), arr(2, 3), arr(1, 2)) == -1      # a 3-wide vertex as intrinsics
    assert run() == -5
    assert analyze(dim, arr(0, 1), arr(2, 3), arr(1, 0)) == -1      # a vertex both camera and intrinsics
    assert analyze(dim, arr(0, 0), arr(2, 4), arr(1, 1)) == -1      # index out of range
    assert analyze(dim, *good, unary=4) == -1
    assert run() == -5
    ctx.close()
