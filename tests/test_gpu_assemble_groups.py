"""Multi-group assembly (spp_assemble_analyze_groups / spp_assemble_groups_device): several edge groups summed into
one Lambda / eta. One group gives the bits of the one-group entry points; two groups are checked against a dense
float64 Lambda built here edge by edge, as tests/test_gpu_schur_2d._problem builds it (bound 1e-13 max|Lambda|, the one
test_range_bearing_group_assembled_and_solved_on_the_device uses for the same comparison)."""
import numpy as np
import pytest

from slam_plus_plus_amd import api, synth
from slam_plus_plus_amd.blockcsc import structure_from_pairs
from oracle import spp_oracle as orc

pytestmark = pytest.mark.gpu


class _Group(dict):
    __getattr__ = dict.__getitem__


def _group_of(prob, sel=None):
    sel = slice(None) if sel is None else sel
    return _Group(v0=prob.v0[sel], v1=prob.v1[sel], d0=prob.d0, d1=prob.d1, rd=prob.rd, J0=prob.J0[sel], J1=prob.J1[sel],
                  Om=prob.Om[sel], r=prob.r[sel])


def _one_group(ctx, prob, damping, unary, weights=None):
    """the existing path: spp_assemble_analyze + spp_assemble_device"""
    st = ctx.assemble_analyze(prob.dim, prob.v0, prob.v1, prob.d0, prob.d1, prob.rd, unary)
    arrs = [api.DeviceArray.from_host(ctx, a.ravel()) for a in (prob.J0, prob.J1, prob.Om, prob.r)]
    dw = None
    if weights is not None:
        dw = api.DeviceArray.from_host(ctx, weights)
        ctx.assemble_set_edge_weights(dw.ptr)
    dv, de = api.DeviceArray(ctx, st.nvals), api.DeviceArray(ctx, st.n)
    ctx.assemble_device(*[a.ptr for a in arrs], damping, dv.ptr, de.ptr)
    out = st, dv.download(), de.download()
    for d in arrs + [dv, de] + ([dw] if dw else []):
        d.free()
    return out


def _groups(ctx, dim, groups, seq, damping, unary, weights=None, weights_by_old_entry=False, repeat=1):
    st = ctx.assemble_analyze_groups(dim, [(g.v0, g.v1, g.d0, g.d1, g.rd) for g in groups], seq, unary)
    arrs = [[api.DeviceArray.from_host(ctx, np.ascontiguousarray(g[k]).ravel()) for g in groups] for k in ("J0", "J1", "Om", "r")]
    dws = []
    for gi, w in enumerate(weights or []):
        if w is None:
            continue
        dws.append(api.DeviceArray.from_host(ctx, w))
        if weights_by_old_entry:
            assert gi == 0
            ctx.assemble_set_edge_weights(dws[-1].ptr)
        else:
            ctx.assemble_set_group_edge_weights(gi, dws[-1].ptr)
    dv, de = api.DeviceArray(ctx, st.nvals), api.DeviceArray(ctx, st.n)
    outs = []
    for _ in range(repeat):
        ctx.assemble_groups_device(*[[a.ptr for a in arr] for arr in arrs], damping, dv.ptr, de.ptr)
        outs.append((dv.download(), de.download()))
    for d in [a for arr in arrs for a in arr] + dws + [dv, de]:
        d.free()
    return (st,) + outs[0] if repeat == 1 else (st, outs)


def _same_structure(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("col_ptr", "row_idx", "blk_off"))


# ---- one group: the bits of the existing path --------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ba_tiny", "se2_small", "se3_small", "lm2d_interleaved"])   # (6,3,2) (3,3,3) (6,6,6) (3,2,2)
def test_one_group_is_bit_identical_to_the_one_group_entry_points(hip_ctx, name):
    prob = synth.make(name)
    g = _group_of(prob)
    for damping, unary in ((0.0, -1), (0.37, -1), (0.0, prob.unary_vertex), (prob.damping + 0.01, prob.unary_vertex)):
        st0, v0, e0 = _one_group(hip_ctx, prob, damping, unary)
        st1, v1, e1 = _groups(hip_ctx, prob.dim, [g], None, damping, unary)
        assert _same_structure(st0, st1)
        assert np.array_equal(v0, v1) and np.array_equal(e0, e1), (name, damping, unary)
    w = np.random.default_rng(3).uniform(0.2, 1.0, size=prob.v0.size)
    st0, v0, e0 = _one_group(hip_ctx, prob, 0.25, prob.unary_vertex, weights=w)
    assert not np.array_equal(v0, _one_group(hip_ctx, prob, 0.25, prob.unary_vertex)[1])   # (the weights are applied at all)
    for by_old_entry in (False, True):
        _, v1, e1 = _groups(hip_ctx, prob.dim, [g], None, 0.25, prob.unary_vertex, [w], weights_by_old_entry=by_old_entry)
        assert np.array_equal(v0, v1) and np.array_equal(e0, e1), (name, by_old_entry)
    # either analyze call resets the weights
    _, v2, e2 = _groups(hip_ctx, prob.dim, [g], None, 0.25, prob.unary_vertex)
    _, v3, e3 = _one_group(hip_ctx, prob, 0.25, prob.unary_vertex)
    assert np.array_equal(v2, v3) and np.array_equal(e2, e3) and not np.array_equal(v2, v0)


def test_one_group_plan_serves_both_device_entry_points(hip_ctx):
    """one plan type: a one-group plan made by spp_assemble_analyze_groups is accepted by spp_assemble_device"""
    prob = synth.make("se2_small")
    st = hip_ctx.assemble_analyze_groups(prob.dim, [(prob.v0, prob.v1, 3, 3, 3)], None, prob.unary_vertex)
    arrs = [api.DeviceArray.from_host(hip_ctx, a.ravel()) for a in (prob.J0, prob.J1, prob.Om, prob.r)]
    dv, de = api.DeviceArray(hip_ctx, st.nvals), api.DeviceArray(hip_ctx, st.n)
    hip_ctx.assemble_device(*[a.ptr for a in arrs], 0.0, dv.ptr, de.ptr)
    _, v0, e0 = _one_group(hip_ctx, prob, 0.0, prob.unary_vertex)
    assert np.array_equal(dv.download(), v0) and np.array_equal(de.download(), e0)
    for d in arrs + [dv, de]:
        d.free()


# ---- two groups against a dense float64 Lambda ---------------------------------------------------------------------
def _random_group(rng, v0, v1, d0, d1, rd):
    ne = len(v0)
    A = rng.normal(size=(ne, rd, rd))
    Om = np.einsum("eij,ekj->eik", A, A) + rd * np.eye(rd)          # SPD information, symmetric
    return _Group(v0=np.asarray(v0, dtype=np.int64), v1=np.asarray(v1, dtype=np.int64), d0=d0, d1=d1, rd=rd,
                  J0=rng.normal(size=(ne, d0 * rd)), J1=rng.normal(size=(ne, d1 * rd)), Om=Om.reshape(ne, rd * rd),
                  r=rng.normal(size=(ne, rd)))


def _dense(dim, groups, damping, unary, weights=None):
    """Lambda and eta edge by edge in float64 (the sum order only moves the last bits, which the bound allows for).
    A robust weight w enters as in the reference (BaseTypes_Binary.h:768-848): H00, H01, H11 and g1 once, g0 twice."""
    base = np.zeros(dim.size + 1, dtype=np.int64)
    np.cumsum(dim, out=base[1:])
    n = int(base[-1])
    L, eta, pairs = np.zeros((n, n)), np.zeros(n), []
    for gi, g in enumerate(groups):
        for e in range(g.v0.size):
            a, b = int(g.v0[e]), int(g.v1[e])
            w = 1.0 if weights is None or weights[gi] is None else weights[gi][e]
            Ja, Jb = g.J0[e].reshape(g.d0, g.rd).T, g.J1[e].reshape(g.d1, g.rd).T      # column-major rd x d
            Om = g.Om[e].reshape(g.rd, g.rd)
            sa, sb = slice(base[a], base[a] + g.d0), slice(base[b], base[b] + g.d1)
            L[sa, sa] += w * (Ja.T @ Om @ Ja)
            L[sb, sb] += w * (Jb.T @ Om @ Jb)
            L[sa, sb] += w * (Ja.T @ Om @ Jb)
            L[sb, sa] += w * (Jb.T @ Om @ Ja)
            eta[sa] += w * w * (Ja.T @ Om @ g.r[e])
            eta[sb] += w * (Jb.T @ Om @ g.r[e])
            pairs.append((min(a, b), max(a, b)))
    L += damping * np.eye(n)
    if unary >= 0:
        L[base[unary]:base[unary + 1], base[unary]:base[unary + 1]] += np.eye(dim[unary])
    rows, cols = np.array(pairs).T
    st, _, _ = structure_from_pairs(dim, rows, cols)
    vals = np.zeros(st.nvals)
    for j in range(st.nb):
        for p in range(st.col_ptr[j], st.col_ptr[j + 1]):
            i = st.row_idx[p]
            blk = L[base[i]:base[i] + dim[i], base[j]:base[j] + dim[j]]
            vals[st.blk_off[p]:st.blk_off[p] + blk.size] = blk.ravel(order="F")
    return st.with_vals(vals), eta


N_POSES, N_LM = 60, 90


def _slam2d_groups(seed=11):
    """(3,3,3) odometry + (3,2,2) observations over interleaved ids, with: one pose pair joined by two odometry edges in
    opposite directions (a shared block, one contribution transposed), pose 0 of degree > 24 fed by both groups (the wave
    kernel across groups), the last landmark of degree 1"""
    rng = np.random.default_rng(seed)
    nv = N_POSES + N_LM
    ids = rng.permutation(nv)
    pose_id, lm_id = ids[:N_POSES], ids[N_POSES:]
    dim = np.empty(nv, dtype=np.int32)
    dim[pose_id], dim[lm_id] = 3, 2
    o0 = list(range(N_POSES - 1)) + [3, 4]
    o1 = list(range(1, N_POSES)) + [4, 3]
    for _ in range(N_POSES // 5):
        i, j = rng.choice(N_POSES, size=2, replace=False)
        o0.append(int(i))
        o1.append(int(j))
    po, lo = [], []
    for l in range(N_LM - 1):
        c = rng.integers(0, N_POSES)
        for p in np.unique(np.clip(c + rng.integers(-6, 7, size=rng.integers(2, 6)), 1, N_POSES - 1)):
            po.append(int(p))
            lo.append(l)
    for l in range(30):                       # pose 0 sees 30 landmarks
        po.append(0)
        lo.append(l)
    po.append(7)                              # the last landmark: one observation
    lo.append(N_LM - 1)
    g_odo = _random_group(rng, pose_id[o0], pose_id[o1], 3, 3, 3)
    g_obs = _random_group(rng, pose_id[po], lm_id[lo], 3, 2, 2)
    deg = np.bincount(np.concatenate([g_odo.v0, g_odo.v1, g_obs.v0, g_obs.v1]), minlength=nv)
    assert deg[pose_id[0]] > 24 and deg[lm_id[-1]] == 1
    assert (g_obs.v1 < g_obs.v0).any() and (g_obs.v1 > g_obs.v0).any()          # transposed and plain blocks
    return dim, [g_odo, g_obs], int(pose_id[0])


def _ba_groups(seed=12):
    """(6,6,6) camera chain + (6,3,2) projections: 12 cameras, 60 points, interleaved ids"""
    rng = np.random.default_rng(seed)
    nc, npts = 12, 60
    ids = rng.permutation(nc + npts)
    cam_id, pt_id = ids[:nc], ids[nc:]
    dim = np.empty(nc + npts, dtype=np.int32)
    dim[cam_id], dim[pt_id] = 6, 3
    co, po = [], []
    for p in range(npts):
        for c in rng.choice(nc, size=rng.integers(2, 5), replace=False):
            co.append(int(c))
            po.append(p)
    g_chain = _random_group(rng, cam_id[np.arange(nc - 1)], cam_id[np.arange(1, nc)], 6, 6, 6)
    g_proj = _random_group(rng, cam_id[co], pt_id[po], 6, 3, 2)
    return dim, [g_chain, g_proj], int(cam_id[0])


def _random_seq(groups, seed):
    perm = np.random.default_rng(seed).permutation(sum(g.v0.size for g in groups))
    cut = np.cumsum([0] + [g.v0.size for g in groups])
    return [perm[cut[i]:cut[i + 1]] for i in range(len(groups))]


@pytest.mark.parametrize("make", [_slam2d_groups, _ba_groups])
def test_two_groups_match_a_dense_float64_lambda(hip_ctx, make):
    dim, groups, unary = make()
    lam, eta = _dense(dim, groups, 1e-2, unary)
    seq = _random_seq(groups, 5)
    st, vals, e = _groups(hip_ctx, dim, groups, seq, 1e-2, unary)
    assert _same_structure(st, lam)
    dv, de = np.abs(vals - lam.vals).max(), np.abs(e - eta).max()
    print("max|dLambda| %.3e (max|Lambda| %.3e), max|deta| %.3e (max|eta| %.3e)" % (dv, np.abs(lam.vals).max(), de, np.abs(eta).max()))
    assert dv <= 1e-13 * np.abs(lam.vals).max()
    assert de <= 1e-13 * np.abs(eta).max()
    # robust weights are per group: the second group weighted, the first plain
    w = [None, np.random.default_rng(8).uniform(0.2, 1.0, size=groups[1].v0.size)]
    lam_w, eta_w = _dense(dim, groups, 1e-2, unary, w)
    _, vw, ew = _groups(hip_ctx, dim, groups, seq, 1e-2, unary, w)
    assert np.abs(vw - lam_w.vals).max() <= 1e-13 * np.abs(lam_w.vals).max()
    assert np.abs(ew - eta_w).max() <= 1e-13 * np.abs(eta_w).max()


def test_without_seq_equals_the_concatenation_and_runs_repeat(hip_ctx):
    dim, groups, unary = _slam2d_groups()
    m = groups[0].v0.size
    st0, (a, b) = _groups(hip_ctx, dim, groups, None, 0.0, unary, repeat=2)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])                   # run to run
    concat = [np.arange(m), m + np.arange(groups[1].v0.size)]
    for seq in (concat, [None, concat[1]]):
        st1, v, e = _groups(hip_ctx, dim, groups, seq, 0.0, unary)
        assert _same_structure(st0, st1) and np.array_equal(v, a[0]) and np.array_equal(e, a[1])
    # another analysis of the same input gives the same bits too
    _, v, e = _groups(hip_ctx, dim, groups, None, 0.0, unary)
    assert np.array_equal(v, a[0]) and np.array_equal(e, a[1])


@pytest.mark.parametrize("name", ["se2_small", "ba_tiny"])
def test_one_shape_split_in_two_groups_keeps_the_bits(hip_ctx, name):
    """even and odd edges as two groups of the same shape, h_seq = the original edge index: every destination sums in
    the original order (ba_tiny: through the wave kernel's butterfly as well), so nothing may change. With robust
    weights the sums are the same sums in the same order, but w * s + sum is contracted into an FMA in some kernels and
    rounded twice in others (measured: se2_small eta differs in last bits, Lambda does not): there the bound is the
    assembly's 1e-13 of the largest entry -- a vertex has at most 24 sequential contributions of one extra rounding
    (1.1e-16) each, the wave kernel's butterfly adds 6 levels."""
    prob = synth.make(name)
    ne = prob.v0.size
    even, odd = np.arange(0, ne, 2), np.arange(1, ne, 2)
    w = np.random.default_rng(4).uniform(0.2, 1.0, size=ne)
    for weights in (None, w):
        st0, v0, e0 = _one_group(hip_ctx, prob, 0.125, prob.unary_vertex, weights)
        st1, v1, e1 = _groups(hip_ctx, prob.dim, [_group_of(prob, even), _group_of(prob, odd)], [even, odd], 0.125,
                              prob.unary_vertex, None if weights is None else [w[even], w[odd]])
        assert _same_structure(st0, st1)
        if weights is None:
            assert np.array_equal(v0, v1) and np.array_equal(e0, e1)
        else:
            print(name, "weighted: max|dLambda| %.3e, max|deta| %.3e" % (np.abs(v0 - v1).max(), np.abs(e0 - e1).max()))
            assert np.abs(v0 - v1).max() <= 1e-13 * np.abs(v0).max() and np.abs(e0 - e1).max() <= 1e-13 * np.abs(e0).max()


def test_union_structure_goes_straight_to_the_solver(hip_ctx):
    dim, groups, unary = _slam2d_groups()
    lam, eta = _dense(dim, groups, 1e-2, unary)
    rows = np.concatenate([np.minimum(g.v0, g.v1) for g in groups])
    cols = np.concatenate([np.maximum(g.v0, g.v1) for g in groups])
    want, _, _ = structure_from_pairs(dim, rows, cols)
    ctx = api.Context(0)
    st = ctx.assemble_analyze_groups(dim, [(g.v0, g.v1, g.d0, g.d1, g.rd) for g in groups], None, unary)
    assert _same_structure(st, want) and st.nvals == want.nvals
    assert ctx.info("NNZB") == want.nnzb and ctx.info("NVALS") == want.nvals
    arrs = [[api.DeviceArray.from_host(ctx, g[k].ravel()) for g in groups] for k in ("J0", "J1", "Om", "r")]
    dv, de = api.DeviceArray(ctx, st.nvals), api.DeviceArray(ctx, st.n)
    ctx.assemble_groups_device(*[[a.ptr for a in arr] for arr in arrs], 1e-2, dv.ptr, de.ptr)
    ctx.analyze(st, api.MODE_AUTO)
    assert ctx.info("MODE") == api.MODE_SCHUR and ctx.info("N_REDUCED") == 3 * N_POSES
    assert ctx.factor_solve_device(dv.ptr, de.ptr) == 0
    code, xo = orc.solve_blocky(lam, eta)
    assert code == 0
    x = de.download()
    assert np.linalg.norm(x - xo) / np.linalg.norm(xo) < 1e-10
    ctx.close()


# ---- errors ----------------------------------------------------------------------------------------------------------
BADARG, STATE, UNSUPPORTED = "spp error -1", "spp error -5", "spp error -6"


def _expect_no_plan(ctx):
    d = api.DeviceArray(ctx, 64)
    with pytest.raises(api.SppError, match=STATE):
        ctx.assemble_groups_device([d.ptr], [d.ptr], [d.ptr], [d.ptr], 0.0, d.ptr, d.ptr)
    with pytest.raises(api.SppError, match=STATE):
        ctx.assemble_device(d.ptr, d.ptr, d.ptr, d.ptr, 0.0, d.ptr, d.ptr)
    d.free()


def test_error_codes():
    ctx = api.Context(0)
    _expect_no_plan(ctx)                                                    # nothing analyzed yet
    dim = np.array([3, 3, 2, 3, 2], dtype=np.int32)
    odo = (np.array([0, 1]), np.array([1, 3]), 3, 3, 3)
    obs = (np.array([0, 3, 1]), np.array([2, 4, 2]), 3, 2, 2)

    def good():
        ctx.assemble_analyze_groups(dim, [odo, obs], None, 0)

    def rejected(code, groups, seq=None):
        good()
        with pytest.raises(api.SppError, match=code):
            ctx.assemble_analyze_groups(dim, groups, seq, 0)

    rejected(UNSUPPORTED, [odo, (obs[0], obs[1], 3, 2, 3)])                 # a shape that is not instantiated
    _expect_no_plan(ctx)
    rejected(UNSUPPORTED, [odo] * 5)                                        # more than SPP_MAX_EDGE_GROUPS
    _expect_no_plan(ctx)
    good()
    with pytest.raises(api.SppError, match=UNSUPPORTED):                    # the one-group entry rejects alike
        ctx.assemble_analyze(dim, obs[0], obs[1], 3, 2, 3, 0)
    _expect_no_plan(ctx)
    for groups, seq in (([odo, (obs[1], obs[0], 3, 2, 2)], None),           # widths do not match the group
                        ([(np.array([0, 1]), np.array([1, 2]), 3, 3, 3), obs], None),
                        ([odo, (np.array([0, 3, 5]), obs[1], 3, 2, 2)], None),      # index out of range
                        ([odo, (np.array([0, -1, 1]), obs[1], 3, 2, 2)], None),
                        ([(np.array([0, 1]), np.array([1, 1]), 3, 3, 3), obs], None),   # a self edge
                        ([odo, obs], [np.array([0, 1]), np.array([2, 3, 3])]),      # h_seq: a repeated position
                        ([odo, obs], [np.array([0, 5]), np.array([2, 3, 4])]),      # h_seq: out of range
                        ([odo, obs], [np.array([1, 2]), None])):                    # h_seq: collides with the default positions
        rejected(BADARG, groups, seq)
        _expect_no_plan(ctx)                                                # after a rejected call: no plan
    good()
    d = api.DeviceArray(ctx, 64)
    with pytest.raises(api.SppError, match=STATE):                          # the one-group entry on a plan of two groups
        ctx.assemble_device(d.ptr, d.ptr, d.ptr, d.ptr, 0.0, d.ptr, d.ptr)
    with pytest.raises(api.SppError, match=BADARG):
        ctx.assemble_set_group_edge_weights(2, d.ptr)
    # a group without edges needs no arrays
    st = ctx.assemble_analyze_groups(dim, [(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), 3, 3, 3), obs], None, 0)
    g = _random_group(np.random.default_rng(1), obs[0], obs[1], 3, 2, 2)
    arrs = [api.DeviceArray.from_host(ctx, g[k].ravel()) for k in ("J0", "J1", "Om", "r")]
    dv, de = api.DeviceArray(ctx, st.nvals), api.DeviceArray(ctx, st.n)
    ctx.assemble_groups_device(*[[None, a.ptr] for a in arrs], 0.0, dv.ptr, de.ptr)
    lam, eta = _dense(dim, [g], 0.0, 0)
    assert np.abs(dv.download() - lam.vals).max() <= 1e-13 * np.abs(lam.vals).max()
    d.free()
    ctx.close()
