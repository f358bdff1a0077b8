"""Deterministic edge fixtures of the Schur stage, built block by block (test infrastructure, numpy only).

Every edge (u, v) contributes J_u^T J_u, J_v^T J_v and J_u^T J_v (unit information), every diagonal block a small
damping; eta = sum J^T r. The landmark side of an observation is J_l = I + 0.25 N(0, 1) (square), so that every landmark
block C stays well conditioned (cond <= 1e2, asserted) and the rounding of C^-1 stays inside the bound of schur_ref.

  edges63       6-wide cameras, 3-wide points (guided Schur), 320 cameras (n_red = 1920 = 15 * 128: the rhs column is
                the first padding column). S blocks of 1, 63, 64, 65, 128, 2047, 2048, 2049 and 4100 pairs (PAIR_CHUNK =
                2048: blocks of more are split over several work items); a camera that observes nothing, tied to another
                by an A block only; an off-diagonal A block without a shared landmark; 300 consecutive single-observation
                landmarks, then 600 of which every 8th is seen by nobody (the `l - first >= 256` cut of the
                back-substitution groups, which only binds before the observation cut when a group holds landmarks
                without observations); a track of exactly 256 observers (the largest one group of the fused
                back-substitution takes)
  edges63_long  the same plus a landmark with 257 observers: no fused back-substitution for this plan
  edges32       3-wide poses, 2-wide landmarks, 128 poses (n_red = 384), the same pair-count spread
  mis66, mis33  one width (MIS Schur cut): two hubs tied to 2100 leaves each (a split S block between the hubs once
                the library eliminates the leaves), plus a chain of 40 vertices hanging off hub 1
  ring()        closed loops and open chains of any widths (loop32 and loop63 here, loop73 and chain73 in schur_fixtures_73.py)
  tiny_shards   4 cameras, 2 landmarks: with 3 landmark shards one owns nothing"""
import numpy as np

from slam_plus_plus_amd.blockcsc import structure_from_pairs

# designated S blocks among cameras 0..4: (camera, camera, shared two-observer landmarks)
PAIR_SPREAD = [(0, 1, 1), (0, 2, 63), (0, 3, 64), (0, 4, 65), (0, 5, 128), (1, 2, 2047), (1, 3, 2048), (2, 4, 2049),
               (3, 4, 4100)]
EDGE_COUNTS = sorted({k for _, _, k in PAIR_SPREAD})
N_SINGLE = 300
N_SPARSE = 600
COND_MAX = 1e2


def _add_blocks(vals, off, di, blocks):
    """vals[off + r + di c] += blocks[:, r, c] for a stack of blocks (any count, duplicates allowed)"""
    n, r_, c_ = blocks.shape
    e = np.arange(r_ * c_)
    idx = off[:, None] + (e % r_)[None, :] + di * (e // r_)[None, :]
    np.add.at(vals, idx.ravel(), blocks[:, e % r_, e // r_].ravel())


def build_system(dim, groups, damping, seed):
    """groups: list of (u, v, Ju, Jv, r) with u, v (n,) block ids of equal widths inside a group, Ju (n, rd, du),
    Jv (n, rd, dv), r (n, rd). Returns (BlockCSC with values, eta)."""
    dim = np.asarray(dim, dtype=np.int32)
    rows = np.concatenate([np.minimum(g[0], g[1]) for g in groups])
    cols = np.concatenate([np.maximum(g[0], g[1]) for g in groups])
    st, blk, dblk = structure_from_pairs(dim, rows, cols)
    vals = np.zeros(st.nvals)
    base = st.base
    eta = np.zeros(st.n)
    at = 0
    for u, v, Ju, Jv, r in groups:
        n = u.size
        b = blk[at:at + n]
        at += n
        du, dv = Ju.shape[2], Jv.shape[2]
        _add_blocks(vals, st.blk_off[dblk[u]], du, np.einsum("nru,nrv->nuv", Ju, Ju))
        _add_blocks(vals, st.blk_off[dblk[v]], dv, np.einsum("nru,nrv->nuv", Jv, Jv))
        up = u < v
        if up.any():
            _add_blocks(vals, st.blk_off[b[up]], du, np.einsum("nru,nrv->nuv", Ju[up], Jv[up]))
        if (~up).any():
            _add_blocks(vals, st.blk_off[b[~up]], dv, np.einsum("nru,nrv->nuv", Jv[~up], Ju[~up]))
        np.add.at(eta, base[u][:, None] + np.arange(du)[None, :], np.einsum("nru,nr->nu", Ju, r))
        np.add.at(eta, base[v][:, None] + np.arange(dv)[None, :], np.einsum("nrv,nr->nv", Jv, r))
    for j in range(st.nb):
        d = int(dim[j])
        p = dblk[j]
        vals[st.blk_off[p]:st.blk_off[p] + d * d].reshape(d, d)[np.diag_indices(d)] += damping
    return st.with_vals(vals), eta


def _guided(nc, nl, dp, dl, obs, a_edges, seed):
    """cameras 0..nc-1 first, landmarks nc..nc+nl-1; obs: (camera, landmark index) pairs; a_edges: (camera, camera)"""
    rng = np.random.default_rng(seed)
    dim = np.array([dp] * nc + [dl] * nl, dtype=np.int32)
    oc = np.array([o[0] for o in obs], dtype=np.int64)
    ol = np.array([o[1] for o in obs], dtype=np.int64) + nc
    n = oc.size
    Jl = np.eye(dl)[None] + 0.25 * rng.standard_normal((n, dl, dl))
    Jc = rng.standard_normal((n, dl, dp))
    groups = [(oc, ol, Jc, Jl, rng.standard_normal((n, dl)))]
    if a_edges:
        au = np.array([a for a, _ in a_edges], dtype=np.int64)
        av = np.array([b for _, b in a_edges], dtype=np.int64)
        m = au.size
        groups.append((au, av, 0.5 * rng.standard_normal((m, dp, dp)), 0.5 * rng.standard_normal((m, dp, dp)),
                       rng.standard_normal((m, dp))))
    return build_system(dim, groups, 1.0, seed)


def _edges_guided(nc, dp, dl, seed, long_track=False, track256=True):
    rng = np.random.default_rng(seed)
    obs = []
    two = []
    for a, b, k in PAIR_SPREAD:
        two += [(a, b)] * k
    two = [two[i] for i in rng.permutation(len(two))]   # the designated pairs interleaved in landmark order
    lm = 0
    for a, b in two:
        obs += [(a, lm), (b, lm)]
        lm += 1
    # N_SINGLE consecutive single-observation landmarks, dealt to cameras 10 .. nc - 3
    for q in range(N_SINGLE):
        obs.append((10 + q % (nc - 12), lm))
        lm += 1
    # then 600 more, every 8th of them seen by nobody: only there can a group reach 257 landmarks with at most 256
    # observations, i.e. only there does the landmark-count cut act alone
    for q in range(N_SPARSE):
        if q % 8 != 7:
            obs.append((10 + q % (nc - 12), lm))
        lm += 1
    if track256:
        obs += [(20 + q, lm) for q in range(256)]
        lm += 1
    if long_track:
        obs += [(20 + q, lm) for q in range(257)]
        lm += 1
    # camera nc - 1 observes nothing and hangs off camera nc - 2 by an A block; (5, nc - 20) is an A block of two cameras
    # without a shared landmark; (1, 3) and (3, 4) are A blocks of an unsplit and of a split pair block
    a_edges = [(nc - 2, nc - 1), (5, nc - 20), (1, 3), (3, 4), (0, 1)]
    return _guided(nc, lm, dp, dl, obs, a_edges, seed)


def edges63():
    return _edges_guided(320, 6, 3, 63)


def edges63_long():
    return _edges_guided(320, 6, 3, 63, long_track=True)


def edges32():
    return _edges_guided(128, 3, 2, 32, track256=False)


def _mis(d, seed, n_leaves=2100, n_chain=40):
    rng = np.random.default_rng(seed)
    nb = 2 + n_leaves + n_chain
    leaves = np.arange(2, 2 + n_leaves)
    chain = np.arange(2 + n_leaves, nb)
    u = np.concatenate([np.zeros(n_leaves, np.int64), np.ones(n_leaves, np.int64), [1], chain[:-1]])
    v = np.concatenate([leaves, leaves, [chain[0]], chain[1:]])
    n = u.size
    Ju = np.eye(d)[None] + 0.25 * rng.standard_normal((n, d, d))
    Jv = np.eye(d)[None] + 0.25 * rng.standard_normal((n, d, d))
    return build_system(np.full(nb, d, dtype=np.int32), [(u, v, Ju, Jv, rng.standard_normal((n, d)))], 1.0, seed)


def mis66():
    return _mis(6, 66)


def mis33():
    return _mis(3, 33)


N_SPLIT = 2100   # landmarks of the designated pair of ring(): more than PAIR_CHUNK = 2048 products, a split S block


def ring_a_edges(nc):
    """the camera-camera blocks of ring(): (u, u + 5) for every 3rd camera u < nc - 5"""
    u = np.arange(0, nc - 5, 3)
    return u, u + 5


def ring(nc, dp, dl, half, per=3, seed=0, split=None, wrap=True):
    """a loop of nc cameras: for every camera c, `per` landmarks, each seen by c and by two distinct cameras c + o1, c + o2
    with offsets drawn from 1..half (indices mod nc; with wrap=False an open chain: a landmark that would reach past the
    last camera is not made); camera-camera blocks ring_a_edges(nc); N_SPLIT more landmarks seen by the two cameras of
    `split` alone, which are tied by a camera-camera block as well"""
    rng = np.random.default_rng(seed)
    obs = []
    lm = 0
    for c in range(nc):
        for _ in range(per):
            o1, o2 = (int(o) for o in 1 + rng.choice(half, 2, replace=False))
            if not wrap and c + max(o1, o2) >= nc:
                continue
            obs += [(c, lm), ((c + o1) % nc, lm), ((c + o2) % nc, lm)]
            lm += 1
    if split is not None:
        for _ in range(N_SPLIT):
            obs += [(split[0], lm), (split[1], lm)]
            lm += 1
    u, v = ring_a_edges(nc)
    a_edges = list(zip(u.tolist(), v.tolist()))
    if split is not None and tuple(split) not in a_edges:   # the split S block carries a camera-camera block too
        a_edges.append(tuple(split))
    return _guided(nc, lm, dp, dl, obs, a_edges, seed)


LOOP32_SPLIT = (135, 140)


def loop32():
    """300 three-wide poses in a loop, 2-wide landmarks (n_red = 900, 8 tile rows; 128 poses per arc-length unit):
    the camera order is accepted, camera-camera blocks in both senses, the split pair reversed
    (tests/test_schur_fixtures_73_host.py asserts it)"""
    return ring(300, 3, 2, half=10, seed=5, split=LOOP32_SPLIT)


LOOP63_SPLIT = (135, 140)


def loop63():
    """300 six-wide cameras in a loop, 3-wide landmarks (n = 10800, n_red = 1800, 15 tile rows; the arc length of this
    width is 64 cameras, 3 tile rows; co-visibility +-8 cameras -- with +-12 the two separators leave no room for two arcs
    of whole tiles and the natural order is kept): the camera order is accepted, camera-camera blocks in both senses
    (tests/test_schur_fixtures_73_host.py asserts it)"""
    return ring(300, 6, 3, half=8, seed=5, split=LOOP63_SPLIT)


def _tiny_shards(dp, seed):
    """4 cameras, 2 landmarks each seen by two cameras, one camera-camera block: with 3 landmark shards rank 2 owns
    no landmark"""
    return _guided(4, 2, dp, 3, [(0, 0), (1, 0), (2, 1), (3, 1)], [(1, 2)], seed)


def tiny_shards():
    return _tiny_shards(6, 46)


GUIDED = {"edges63": edges63, "edges63_long": edges63_long, "edges32": edges32}
MIS = {"mis66": mis66, "mis33": mis33}
ALL = dict(GUIDED, **MIS)
SHAPES = {"loop32": loop32, "loop63": loop63, "tiny_shards": tiny_shards}   # (not edge fixtures: no pair-count spread)


def make(name):
    return (ALL[name] if name in ALL else SHAPES[name])()


def landmark_conds(lam, elim):
    """condition numbers of the diagonal blocks of the eliminated set"""
    out = []
    for b in elim:
        p = lam.col_ptr[b + 1] - 1
        d = int(lam.dim[b])
        C = lam.vals[lam.blk_off[p]:lam.blk_off[p] + d * d].reshape(d, d)
        out.append(np.linalg.cond(C))
    return np.array(out)
