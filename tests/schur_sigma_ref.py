"""Reference machinery of the Schur selected-inversion tests (test infrastructure, numpy / scipy on the host only):
Sigma = Lambda^-1 on the stored pattern of Lambda for bundle-adjustment systems, by the block formulas

    Lambda = [A W; W^T C],  S = A - W C^-1 W^T,  Z = S^-1
    Sigma[c_i, l] = -(sum_j Z[c_i, c_j] U_j) C_l^-1
    Sigma[l, l]   = C_l^-1 + C_l^-1 (sum_i U_i^T H_i) C_l^-1,   H_i = sum_j Z[c_i, c_j] U_j

reference(name)   S from Lambda's blocks in float64; its inverse refined twice with the residual in longdouble as
                  sparse_sigma_ref.refined_inverse does (exact_product below forms that residual from float64 products that
                  are exact, 70 s -> 3 s at the 1920 reduced rows of edges63_long); C^-1 and the landmark formulas in
                  longdouble; the result in the layout of vals (float64), every stored double.
full_inverse_on_pattern(name)  the same blocks from the refined longdouble inverse of the whole dense Lambda (small fixtures).
Cameras are the vertices of the larger width, wherever they stand in Lambda's numbering (ba_interleaved). Everything is
cached per fixture: the GPU tests share one reference and never change it."""
import numpy as np

import solve_again_ref as sar
import sparse_sigma_ref as sgr

LD = np.longdouble
FIXTURES = ["tiny_shards", "chain73", "loop32", "loop63", "edges63_long", "edges73_aligned", "ba_interleaved"]
FULL = ["tiny_shards", "chain73", "loop32", "loop63"]   # every stored block is also compared with the solve route
N_ALL = 11000                                             # up to this n every block column is checked

_CACHE = {}


def problem(name):
    if name != "ba_interleaved":
        return sar.problem(name)
    if ("p", name) not in _CACHE:
        from slam_plus_plus_amd import synth
        from oracle import spp_oracle as orc
        _CACHE[("p", name)] = orc.assemble(synth.make(name))
    return _CACHE[("p", name)]


def _slices(M, axis, bits, count):
    """M = sum of `count` float64 slices (+ a remainder below 2^-(bits count) of the largest entry along `axis`), every
    slice a multiple of 2^(e - bits) with |.| <= 2^e, e fixed along `axis`: products of two slices sum exactly"""
    out, rest = [], M.copy()
    for _ in range(count):
        mx = np.max(np.abs(rest), axis=axis, keepdims=True)
        e = np.ceil(np.log2(np.where(mx > 0, mx, 1.0)))
        sigma = np.ldexp(0.75, (e + 53 - bits).astype(np.int64))
        hi = (rest + sigma) - sigma
        out.append(hi)
        rest = rest - hi
    return out


def exact_product(S, X):
    """S X in longdouble for a float64 S and a longdouble X (n up to 4096): both are cut into slices of 18 bits whose
    float64 products are exact, and the products are summed in longdouble, smallest first. What is dropped is below
    2^-72 of (row maximum of S) x (column maximum of X) per term"""
    n = S.shape[1]
    assert n <= 4096
    bits = 18   # 2 * 18 + 12 + 2 <= 53
    X1 = X.astype(np.float64)
    X2 = (X - X1.astype(LD)).astype(np.float64)
    Ss = _slices(S, 1, bits, 4)
    terms = []
    for Xp, depth in ((X1, 4), (X2, 1)):
        Xs = _slices(Xp, 0, bits, depth)
        for a in range(len(Ss)):
            for b in range(len(Xs)):
                if a + b <= 3:
                    terms.append((a + b + (0 if Xp is X1 else 3), Ss[a] @ Xs[b]))
    out = np.zeros(S.shape[:1] + X.shape[1:], dtype=LD)
    for _, P in sorted(terms, key=lambda t: -t[0]):
        out += P.astype(LD)
    return out


def refined_inverse(L, passes=sgr.REFINE):
    """sparse_sigma_ref.refined_inverse with the residual's product formed by exact_product"""
    import scipy.linalg as sla
    cf = sla.cho_factor(L)
    eye = np.eye(L.shape[0], dtype=LD)
    X = sla.cho_solve(cf, np.eye(L.shape[0])).astype(LD)
    for _ in range(passes):
        X = X + sla.cho_solve(cf, (eye - exact_product(L, X)).astype(np.float64)).astype(LD)
    return X


class Parts:
    """the blocks of Lambda sorted into cameras, landmarks and observations"""

    def __init__(self, lam):
        dim = lam.dim
        self.dp, self.dl = int(dim.max()), int(dim.min())
        assert self.dp > self.dl
        is_cam = dim == self.dp
        self.cams, self.lms = np.flatnonzero(is_cam), np.flatnonzero(~is_cam)
        rank = np.zeros(lam.nb, dtype=np.int64)
        rank[self.cams] = np.arange(self.cams.size)
        rank[self.lms] = np.arange(self.lms.size)
        self.rank = rank
        i, j = lam.row_idx, lam.col_idx
        ci, cj = is_cam[i], is_cam[j]
        self.cc = np.flatnonzero(ci & cj)                 # camera-camera blocks (upper, incl. diagonal)
        self.ll = np.flatnonzero(~ci & ~cj)
        assert np.array_equal(i[self.ll], j[self.ll]), "landmarks are tied to each other"
        self.ob = np.flatnonzero(ci ^ cj)
        tr = ~ci[self.ob]                                 # stored landmark row first
        cam = np.where(tr, j[self.ob], i[self.ob])
        lm = np.where(tr, i[self.ob], j[self.ob])
        order = np.lexsort((rank[cam], rank[lm]))         # by landmark, then by camera
        self.ob, self.tr = self.ob[order], tr[order]
        self.ob_cam, self.ob_lm = rank[cam[order]], rank[lm[order]]
        dp, dl = self.dp, self.dl
        B = lam.vals[lam.blk_off[self.ob][:, None] + np.arange(dp * dl)[None, :]]
        self.U = np.where(self.tr[:, None, None], B.reshape(-1, dp, dl), B.reshape(-1, dl, dp).transpose(0, 2, 1))
        Cb = lam.vals[lam.blk_off[self.ll][:, None] + np.arange(dl * dl)[None, :]].reshape(-1, dl, dl)
        self.C = np.empty((self.lms.size, dl, dl))
        self.C[rank[i[self.ll]]] = np.triu(Cb.transpose(0, 2, 1)) + np.triu(Cb.transpose(0, 2, 1), 1).transpose(0, 2, 1)
        # every ordered pair of observations of one landmark
        cnt = np.bincount(self.ob_lm, minlength=self.lms.size)
        start = np.zeros(self.lms.size + 1, dtype=np.int64)
        np.cumsum(cnt, out=start[1:])
        k = cnt[self.ob_lm]
        self.pa = np.repeat(np.arange(self.ob.size), k)
        first = np.zeros(self.ob.size + 1, dtype=np.int64)
        np.cumsum(k, out=first[1:])
        self.pb = start[self.ob_lm[self.pa]] + np.arange(self.pa.size) - first[self.pa]


def _cinv(C):
    """C^-1 per landmark in longdouble: numpy's inverse with two Newton steps in longdouble"""
    X = np.linalg.inv(C).astype(LD)
    Cl = C.astype(LD)
    eye = np.eye(C.shape[1], dtype=LD)[None]
    for _ in range(2):
        X = X + np.einsum("lab,lbc->lac", X, eye - np.einsum("lab,lbc->lac", Cl, X))
    return X


def reduced_system(lam, P):
    """dense S = A - W C^-1 W^T in float64, cameras in Lambda's order"""
    dp = P.dp
    nc = P.cams.size
    S4 = np.zeros((nc, nc, dp, dp))
    i, j = P.rank[lam.row_idx[P.cc]], P.rank[lam.col_idx[P.cc]]
    A = lam.vals[lam.blk_off[P.cc][:, None] + np.arange(dp * dp)[None, :]].reshape(-1, dp, dp).transpose(0, 2, 1)
    S4[i, j] = A
    off = i != j
    S4[j[off], i[off]] = A[off].transpose(0, 2, 1)
    Ci = np.linalg.inv(P.C)
    T = np.einsum("prd,pde,pse->prs", P.U[P.pa], Ci[P.ob_lm[P.pa]], P.U[P.pb])
    np.subtract.at(S4, (P.ob_cam[P.pa], P.ob_cam[P.pb]), T)
    S = S4.transpose(0, 2, 1, 3).reshape(nc * dp, nc * dp)
    return np.triu(S) + np.triu(S, 1).T


def formulas(lam, P, Z):
    """the stored blocks of Sigma from Z = S^-1 (longdouble, cameras in Lambda's order), in the layout of vals"""
    dp, dl = P.dp, P.dl
    nc = P.cams.size
    out = np.full(lam.nvals, np.nan)
    Z4 = Z.reshape(nc, dp, nc, dp).transpose(0, 2, 1, 3)
    i, j = P.rank[lam.row_idx[P.cc]], P.rank[lam.col_idx[P.cc]]
    out[lam.blk_off[P.cc][:, None] + np.arange(dp * dp)[None, :]] = Z4[i, j].transpose(0, 2, 1).reshape(-1, dp * dp).astype(np.float64)
    Ul = P.U.astype(LD)
    Ci = _cinv(P.C)
    H = np.zeros((P.ob.size, dp, dl), dtype=LD)
    np.add.at(H, P.pa, np.einsum("prs,psd->prd", Z4[P.ob_cam[P.pa], P.ob_cam[P.pb]], Ul[P.pb]))
    X = -np.einsum("ord,ode->ore", H, Ci[P.ob_lm])                       # Sigma[c, l], dp x dl
    Xs = np.where(P.tr[:, None], X.reshape(-1, dp * dl), X.transpose(0, 2, 1).reshape(-1, dp * dl))
    out[lam.blk_off[P.ob][:, None] + np.arange(dp * dl)[None, :]] = Xs.astype(np.float64)
    M = np.zeros((P.lms.size, dl, dl), dtype=LD)
    np.add.at(M, P.ob_lm, np.einsum("ord,ore->ode", Ul, H))
    D = Ci + np.einsum("lab,lbc,lcd->lad", Ci, M, Ci)
    li = P.rank[lam.row_idx[P.ll]]
    out[lam.blk_off[P.ll][:, None] + np.arange(dl * dl)[None, :]] = D[li].transpose(0, 2, 1).reshape(-1, dl * dl).astype(np.float64)
    assert not np.any(np.isnan(out))
    return out


def parts(name):
    if ("parts", name) not in _CACHE:
        _CACHE[("parts", name)] = Parts(problem(name)[0])
    return _CACHE[("parts", name)]


def reference(name):
    """Sigma on the pattern of Lambda, NVALS float64"""
    if ("ref", name) not in _CACHE:
        lam = problem(name)[0]
        P = parts(name)
        _CACHE[("ref", name)] = formulas(lam, P, refined_inverse(reduced_system(lam, P)))
    return _CACHE[("ref", name)]


def full_inverse_on_pattern(name):
    lam = problem(name)[0]
    return sgr.blocks_on_pattern(lam, refined_inverse(lam.to_scipy().toarray()).astype(np.float64))


def selection(name):
    """vertices whose block columns are sampled on the large fixtures: the first, last (blind) and tile-straddling camera,
    the degree-1, 256-track, 257-track and unobserved landmarks where the fixture has them"""
    lam = problem(name)[0]
    P = parts(name)
    deg = np.bincount(P.ob_lm, minlength=P.lms.size)
    across = np.flatnonzero((lam.base[P.cams] < 128) & (lam.base[P.cams] + P.dp > 128))
    sel = [int(P.cams[0]), int(P.cams[-1])] + [int(P.cams[q]) for q in across[:1]]
    for k in (1, 256, 257, 0):
        hit = np.flatnonzero(deg == k)
        if hit.size:
            sel.append(int(P.lms[hit[0]]))
    return sorted(set(sel))


def checked_vertices(name):
    """the block columns the GPU test compares: all of them up to N_ALL scalars, else every camera and selection()"""
    lam = problem(name)[0]
    if lam.n <= N_ALL:
        return np.arange(lam.nb, dtype=np.int64)
    P = parts(name)
    return np.array(sorted(set(P.cams.tolist()) | set(selection(name))), dtype=np.int64)
