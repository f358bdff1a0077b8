"""Reference machinery of the selected-inversion tests of the SPARSE path (test infrastructure, numpy / scipy on the host
only): Sigma = Lambda^-1 on the stored pattern of Lambda for the systems of tests/sparse_solve_ref.py.

full_inverse(name)   per connected component of a designed fixture with at most FULL_MAX scalars, and for the dense Lambda
                     of se2_small / se3_small at ssr.POSE_DAMPING: the float64 Cholesky inverse refined twice with the
                     residual in longdouble, X <- X + Lambda^-1 (I - Lambda X), kept in longdouble. Measured on the host:
                     max |I - Lambda X| <= 2e-18 on every such component (the 692-wide tree_mid 3.3 s, all of forest_b
                     1.8 s); tests/test_sparse_sigma_ref_host.py asserts 1e-16.
larger components    (tree_hi: 872 scalars, the 1023- and 1024-wide cliques of forest_c): ssr.refined_columns on the unit
                     columns of sampled vertices -- the first, middle and last block of every clique of the component.
checked_vertices     the block columns a reference exists for: all of the former, the sampled ones of the latter.
reference_on_pattern the reference in the layout of vals, NaN where none exists.
blocks_on_pattern    the vals-layout image of a dense matrix; pattern_index the map behind it.
Everything is cached per system: the GPU tests share one reference and never change it."""
import numpy as np

import solve_again_ref as sar
import sparse_solve_ref as ssr

FULL_MAX = 700
REFINE = 2

_CACHE = {}


def pattern_index(lam):
    """per stored double of a BlockCSC: (its offset in vals, its scalar row, its scalar column, its block column)"""
    di = lam.dim[lam.row_idx].astype(np.int64)
    dj = lam.dim[lam.col_idx].astype(np.int64)
    cnt = di * dj
    blk = np.repeat(np.arange(lam.nnzb), cnt)
    start = np.zeros(lam.nnzb + 1, dtype=np.int64)
    np.cumsum(cnt, out=start[1:])
    e = np.arange(int(cnt.sum()), dtype=np.int64) - start[blk]
    r = lam.base[lam.row_idx][blk] + e % di[blk]
    c = lam.base[lam.col_idx][blk] + e // di[blk]
    return lam.blk_off[blk] + e, r, c, lam.col_idx[blk]


def blocks_on_pattern(lam, Sigma):
    """the blocks of the dense n x n matrix Sigma at the stored blocks of lam, in the layout of lam.vals"""
    pos, r, c, _ = pattern_index(lam)
    out = np.full(lam.nvals, np.nan)
    out[pos] = Sigma[r, c]
    return out


def components(name):
    """[(scalar indices, block ids, dense Lambda or None)]: the connected components (a pose graph: one, the dense Lambda);
    the dense matrix only where the full inverse is taken"""
    if ("c", name) not in _CACHE:
        lam = ssr.problem(name)[0]
        if name in ssr.POSE:
            out = [(np.arange(lam.n), np.arange(lam.nb), lam.to_scipy().toarray())]
        else:
            fx = ssr.fixture(name)
            out = [(s, b, L if s.size <= FULL_MAX else None) for s, b, L in zip(fx.comp_scalars, fx.comp_blocks, fx.dense)]
        _CACHE[("c", name)] = out
    return _CACHE[("c", name)]


def refined_inverse(L, passes=REFINE):
    """longdouble X with Lambda X = I: the float64 Cholesky inverse, refined with the residual in longdouble"""
    import scipy.linalg as sla
    cf = sla.cho_factor(L)
    Ll = L.astype(np.longdouble)
    eye = np.eye(L.shape[0], dtype=np.longdouble)
    X = sla.cho_solve(cf, np.eye(L.shape[0])).astype(np.longdouble)
    for _ in range(passes):
        X = X + sla.cho_solve(cf, (eye - Ll @ X).astype(np.float64)).astype(np.longdouble)
    return X


def full_inverse(name):
    """[(scalar indices, longdouble inverse)] of the components the full inverse is taken of"""
    if ("inv", name) not in _CACHE:
        _CACHE[("inv", name)] = [(s, refined_inverse(L)) for s, _, L in components(name) if L is not None]
    return _CACHE[("inv", name)]


def sampled_vertices(name):
    """of the components too large for the full inverse: the first, middle and last block of every clique"""
    if name in ssr.POSE:
        return []
    fx = ssr.fixture(name)
    large = [i for i, (_, _, L) in enumerate(components(name)) if L is None]
    out = []
    for g in fx.cliques:
        if g["comp"] in large:
            b = g["blocks"]
            out += [int(b[0]), int(b[b.size // 2]), int(b[-1])]
    return sorted(set(out))


def checked_vertices(name):
    """the block columns of Sigma the reference covers, ascending"""
    full = [b for _, b, L in components(name) if L is not None]
    return np.array(sorted(set(int(v) for b in full for v in b) | set(sampled_vertices(name))), dtype=np.int64)


def reference_on_pattern(name):
    """the reference Sigma in the layout of vals (float64), NaN at the stored blocks of unchecked block columns"""
    if ("ref", name) not in _CACHE:
        lam = ssr.problem(name)[0]
        pos, r, c, _ = pattern_index(lam)
        ref = np.full(lam.nvals, np.nan)
        loc = np.zeros(lam.n, dtype=np.int64)
        for s, X in full_inverse(name):
            inside = np.zeros(lam.n, dtype=bool)
            inside[s] = True
            loc[s] = np.arange(s.size)
            m = inside[c]          # (a stored block lies inside one component: its row is there too)
            ref[pos[m]] = X[loc[r[m]], loc[c[m]]].astype(np.float64)
        sv = sampled_vertices(name)
        if sv:
            E, rows = sar.unit_columns(lam, sv)
            X = ssr.refined_columns(name, E)
            at = np.full(lam.n, -1, dtype=np.int64)
            at[rows] = np.arange(rows.size)
            m = at[c] >= 0
            ref[pos[m]] = X[r[m], at[c[m]]]
        _CACHE[("ref", name)] = ref
    return _CACHE[("ref", name)]


def column_errors(lam, sigma, ref):
    """per block column: the Frobenius norm of sigma - ref over that of ref on the column's stored blocks (NaN where the
    reference has none)"""
    pos, _, _, cb = pattern_index(lam)
    have = ~np.isnan(ref[pos])
    d = np.where(have, sigma[pos] - ref[pos], 0.0)
    num = np.bincount(cb, d * d, minlength=lam.nb)
    den = np.bincount(cb, np.where(have, ref[pos], 0.0) ** 2, minlength=lam.nb)
    cnt = np.bincount(cb, have, minlength=lam.nb)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(cnt > 0, np.sqrt(num / den), np.nan)
