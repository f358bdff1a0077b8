"""Host-only: the longdouble Schur reference (tests/schur_ref.py) against two independent float64 computations, and the
edge fixtures (tests/schur_fixtures.py) against the edges they exist for, as the host plan sees them (spp_schur_plan_host:
work items, split blocks) -- a change of the generator or of PAIR_CHUNK cannot drop coverage silently. No GPU needed."""
import numpy as np
import pytest
import scipy.sparse as sp

import schur_fixtures as fx
import schur_ref
from slam_plus_plus_amd import api, synth
from oracle import spp_oracle as orc

PAIR_CHUNK = 2048   # spp_schur_plan.cpp: block products per work item of the S accumulation
BS_OBS = 256        # spp_schur_plan.cpp: observations (and landmarks) per group of the fused back-substitution

_CACHE = {}


def _problem(name):
    if name not in _CACHE:
        _CACHE[name] = fx.make(name) if name in fx.ALL else orc.assemble(synth.make(name))
    return _CACHE[name]


def _upper_cov(R):
    n, dp = R.n_red, R.dp
    cov = np.zeros((n, n), dtype=bool)
    for i1, i2 in R.pattern:
        cov[i1 * dp:(i1 + 1) * dp, i2 * dp:(i2 + 1) * dp] = True
    return cov


def _float64_schur(lam, eta, R):
    """S and rhs of the shard in float64 through scipy.sparse (no per-pair loop: a second, differently ordered sum)"""
    A = lam.to_scipy().tocsr()
    P = schur_ref.pose_index(lam, R.poses)
    L = schur_ref.pose_index(lam, R.lms)
    Cinv = sp.block_diag([np.linalg.inv(c) for c in R.C], format="csr") if R.lms.size else sp.csr_matrix((0, 0))
    B = A[P][:, L]
    S = -(B @ Cinv @ B.T).toarray()
    rhs = -(B @ (Cinv @ eta[L]))
    return S, rhs


def _check_upper(R, S, rhs):
    cov = _upper_cov(R)
    kk = R._elem_k()
    ratio = schur_ref._within(S[cov], R.S[cov], R.bound(R.M[cov], kk[cov]), "S")
    return max(ratio, schur_ref._within(rhs, R.rhs, R.bound(R.Mrhs, np.repeat(R.obs_count, R.dp)), "rhs"))


@pytest.mark.parametrize("name,world", [("ba_small", 1), ("ba_small", 2), ("ba_small", 3), ("edges63", 1), ("edges63", 3),
                                        ("edges63_long", 2)])
def test_reference_matches_the_oracle_partial_schur(name, world):
    """orc.schur_partial: the C restatement of the reference's Schur product (3-wide landmarks), shard by shard"""
    lam, eta = _problem(name)
    for rank in range(world):
        R = schur_ref.schur_ref(lam, eta, schur_ref.guided_elim(lam), rank, world)
        S, xred, pidx, mine = orc.schur_partial(lam, eta, rank, world)
        assert np.array_equal(mine, R.lms) and np.array_equal(pidx, schur_ref.pose_index(lam, R.poses))
        ratio = _check_upper(R, S, xred)
        assert ratio <= 1.0
    if world == 1:
        st, _, S2 = orc.schur_solve(lam, eta, want_S=True)
        assert st == 0 and np.array_equal(S2, S)


@pytest.mark.parametrize("name,world", [("lm2d_small", 1), ("lm2d_small", 2), ("edges32", 1), ("edges32", 2), ("ba_small", 1),
                                        ("edges63", 1)])
def test_reference_matches_a_sparse_float64_product(name, world):
    lam, eta = _problem(name)
    for rank in range(world):
        R = schur_ref.schur_ref(lam, eta, schur_ref.guided_elim(lam), rank, world)
        S, rhs = _float64_schur(lam, eta, R)
        if rank == 0:
            P = schur_ref.pose_index(lam, R.poses)
            A = lam.to_scipy().tocsr()[P][:, P].toarray()
            S = S + A
            rhs = rhs + eta[P]
        cov = _upper_cov(R)
        kk = R._elem_k()
        schur_ref._within(S[cov], R.S[cov], R.bound(R.M[cov], kk[cov]), "S")
        schur_ref._within(rhs, R.rhs, R.bound(R.Mrhs, np.repeat(R.obs_count, R.dp)), "rhs")
        assert np.all(S[~cov & np.triu(np.ones_like(cov, dtype=bool))] == 0.0)


def _expected_items(R):
    """work items and split blocks the plan must make of the pattern: one item per PAIR_CHUNK block products"""
    k = np.array([R.k_all[i1, i2] for i1, i2 in R.pattern])
    return int(np.maximum(1, (k + PAIR_CHUNK - 1) // PAIR_CHUNK).sum()), int((k > PAIR_CHUNK).sum())


@pytest.mark.parametrize("name", sorted(fx.GUIDED))
def test_guided_fixture_reaches_its_edges(name):
    lam, eta = _problem(name)
    el = schur_ref.guided_elim(lam)
    R = schur_ref.schur_ref(lam, eta, el)
    nc = R.poses.size
    ku = R.k[np.triu_indices(nc, 1)]
    for k in fx.EDGE_COUNTS:   # 1, 63, 64, 65, 128, 2047, 2048, 2049 pairs and one block of >= 2 PAIR_CHUNK + 1
        assert np.any(ku == k), (name, k)
    assert ku.max() >= 2 * PAIR_CHUNK + 1
    assert R.n_red % 128 == 0, "n_red a multiple of 128: the rhs column of the dense S is the first padding column"
    # a camera that observes nothing, tied to another only by an A block
    blind = np.flatnonzero(R.obs_count == 0)
    assert any(R.has_A[:, c].sum() + R.has_A[c, :].sum() - 2 * R.has_A[c, c] > 0 for c in blind)
    # an off-diagonal A block of two cameras without a shared landmark
    off = np.triu(R.has_A, 1) & (R.k_all == 0)
    assert off.sum() >= 2
    track = np.diff(R.lm_ptr)
    assert np.any(track == 0) and np.any(track == 1), "a landmark seen by nobody, landmarks seen once"
    run = best = 0
    for t in track:
        run = run + 1 if t == 1 else 0
        best = max(best, run)
    assert best >= BS_OBS, "consecutive single-observation landmarks"
    # the groups of the fused back-substitution (spp_schur_plan.cpp): some group must be cut by its landmark count alone
    first, by_count = 0, 0
    for l in range(track.size):
        if R.lm_ptr[l + 1] - R.lm_ptr[first] > BS_OBS or l - first >= BS_OBS:
            by_count += R.lm_ptr[l + 1] - R.lm_ptr[first] <= BS_OBS
            first = l
    assert by_count > 0, "no group of the back-substitution is cut by its landmark count"
    assert track.max() == {"edges63": 256, "edges63_long": 257, "edges32": track.max()}[name]
    assert fx.landmark_conds(lam, el).max() <= fx.COND_MAX
    # the plan: every pair, the expected work items, split blocks
    for sparse in (False, True):
        d = api.schur_plan_host(lam, sparse_S=sparse)
        n_items, n_multi = _expected_items(R)
        assert d["nc"] == nc and d["nl"] == R.lms.size and d["no"] == R.obs_pose.size
        assert d["n_pairs"] == int((track * (track + 1) // 2).sum())
        assert d["n_sblk"] == len(R.pattern)
        assert (d["n_items"], d["n_multi"]) == (n_items, n_multi)
        assert d["n_multi"] > 0
        print(name, "sparse" if sparse else "dense", d)


@pytest.mark.parametrize("name", sorted(fx.MIS))
def test_mis_fixture_reaches_its_edges(name):
    lam, eta = _problem(name)
    d = api.schur_plan_host(lam, mis=True)
    print(name, d)
    assert d["n_multi"] > 0, "the hub-hub block is split over several work items"
    assert d["nc"] + d["nl"] == lam.nb and d["nl"] >= 2100
    assert d["n_pairs"] > 2 * PAIR_CHUNK + 1
    with pytest.raises(api.SppError):   # the guided cut needs two widths
        api.schur_plan_host(lam)


@pytest.mark.parametrize("compact", [False, True])
def test_buffer_check_fails_on_what_the_library_may_get_wrong(compact):
    """check_schur_buffer itself: an entry left at a NaN prefill, a foreign block of a shard that is not exactly 0.0, a
    non-zero below the upper blocks of the dense S and one dropped block product all fail; the exact layouts pass"""
    lam, eta = _problem("edges32")
    R = schur_ref.schur_ref(lam, eta, schur_ref.guided_elim(lam), 1, 2)
    ld = schur_ref.dense_ld(R.n_red)
    dval, _, _, cov = R.dense_layout(ld)
    sval, _, _ = R.sparse_layout()
    dense, sparse = dval.astype(np.float64), sval.astype(np.float64)
    foreign = [q for q, (i1, i2) in enumerate(R.pattern) if R.k[i1, i2] == 0 and not (i1 == i2)]
    assert foreign, "rank 1 of 2 holds blocks that only rank 0's landmarks reach"
    blk = R.dp * R.dp
    if compact:
        R.compact()
    assert schur_ref.check_schur_buffer(R, dense, False, ld) <= 1.0
    assert schur_ref.check_schur_buffer(R, sparse, True) <= 1.0
    bad = []
    b = sparse.copy()
    b[foreign[0] * blk:(foreign[0] + 1) * blk] = np.nan                      # a foreign block never written
    bad.append((b, True))
    b = sparse.copy()
    b[foreign[-1] * blk] = 1e-300                                             # a foreign block not exactly zero
    bad.append((b, True))
    b = sparse.copy()
    b[-1] = np.nan                                                            # an rhs entry never written
    bad.append((b, True))
    b = dense.copy()
    b[np.flatnonzero(cov)[7]] = np.nan                                        # a covered dense entry never written
    bad.append((b, False))
    b = dense.copy()
    b[np.flatnonzero(~cov)[3]] = 1e-300                                       # below the upper blocks
    bad.append((b, False))
    i1, i2 = R.pattern[int(np.argmax([R.k[p] for p in R.pattern]))]          # one product of the fullest block dropped
    o = np.flatnonzero(R.obs_pose == i1)[0]
    prod = (R.obs_B[o] @ R.Cinv[R.obs_lm[o]].astype(np.float64) @ R.obs_B[o].T) if i1 == i2 else None
    b = dense.copy().reshape(ld, ld).T
    b[i1 * R.dp:(i1 + 1) * R.dp, i2 * R.dp:(i2 + 1) * R.dp] += prod if prod is not None else 1.0
    bad.append((b.T.ravel(), False))
    for q, (buf, sp_) in enumerate(bad):
        with pytest.raises(AssertionError):
            schur_ref.check_schur_buffer(R, buf, sp_, 0 if sp_ else ld)
            print("case", q, "passed")
