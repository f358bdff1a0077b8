"""High-precision reference of the Schur stage (test infrastructure, pure numpy).

For a block-CSC Lambda (upper block triangle), eta and a set of eliminated blocks E (block diagonal part C, the
landmarks), the reduced system over the remaining blocks P (the poses, numbered by ascending block index) is

    S   = A - sum_l B_l C_l^-1 B_l^T          (A = Lambda_PP, B_l = Lambda_P,l)
    rhs = eta_P - sum_l B_l C_l^-1 eta_l

accumulated in np.longdouble, observation by observation (never through a dense Lambda). With (rank, world) only the
landmarks of one shard enter (orc.landmark_shard: round-robin over the eliminated blocks in ascending order), and only
rank 0 adds A and eta_P.

Beside the values: the pair count k_ij of every block of S (landmarks observed by both poses), the elementwise
magnitudes M = |A| + sum_l |B_il| |C_l^-1| |B_jl|^T (and |eta_i| + sum_l |B_il| |C_l^-1| |eta_l| for the rhs) and the
upper block pattern of S. A float64 S computed in ANY summation order satisfies

    |S - S_ref| <= 4 (k_ij + 8 dl) eps M_ij

(k_ij + 8 dl: the additions of the pair sum plus the rounding of one product and of C^-1 on a well-conditioned C), so a
test against this bound does not pin today's order, while one dropped pair moves an entry by about M / k."""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)


def _inv_batched(C):
    """inverse of a stack of small SPD blocks (n, d, d) in longdouble: Gauss-Jordan with partial pivoting"""
    n, d, _ = C.shape
    a = C.astype(LD).copy()
    b = np.broadcast_to(np.eye(d, dtype=LD), (n, d, d)).copy()
    rows = np.arange(n)
    for k in range(d):
        piv = k + np.argmax(np.abs(a[:, k:, k]), axis=1)
        for m in (a, b):
            t = m[rows, k].copy()
            m[rows, k] = m[rows, piv]
            m[rows, piv] = t
        p = a[:, k, k][:, None].copy()
        a[:, k] /= p
        b[:, k] /= p
        f = a[:, :, k].copy()
        f[:, k] = 0
        a -= f[:, :, None] * a[:, k][:, None, :]
        b -= f[:, :, None] * b[:, k][:, None, :]
    return b


def _blocks(lam, ps, di, dj):
    """stack of blocks ps, all di x dj as stored"""
    ps = np.asarray(ps, dtype=np.int64)
    idx = lam.blk_off[ps][:, None] + np.arange(di * dj)[None, :]
    return lam.vals[idx].reshape(-1, dj, di).transpose(0, 2, 1)


class SchurRef:
    """Attributes: dp, dl, poses (block index of every pose), lms (eliminated blocks of this shard), n_red,
    S, M (n_red x n_red longdouble, full symmetric), rhs, Mrhs (n_red), k (nc x nc pair counts of this shard),
    k_all (nc x nc over all landmarks), has_A (nc x nc, upper), obs_count (nc: observations of the shard's landmarks),
    pattern (list of upper blocks (i1, i2) of S, i1 <= i2, ascending by (i2, i1)), the shard's observations sorted by
    (landmark, pose) (obs_pose, obs_lm, obs_B: the dp x dl block B_il) with lm_ptr, and per landmark C and Cinv."""

    def __init__(self, lam, eta, elim, rank=0, world=1):
        assert lam.vals is not None
        nb = lam.nb
        is_e = np.zeros(nb, dtype=bool)
        is_e[np.asarray(list(elim), dtype=np.int64)] = True
        poses = np.flatnonzero(~is_e)
        lms_all = np.flatnonzero(is_e)
        dps, dls = np.unique(lam.dim[poses]), np.unique(lam.dim[lms_all])
        assert dps.size == 1 and dls.size == 1, "one pose width and one landmark width"
        dp, dl = int(dps[0]), int(dls[0])
        self.dp, self.dl, self.poses = dp, dl, poses
        self.rank, self.world = rank, world
        nc = poses.size
        self.n_red = n_red = nc * dp
        pose_of = -np.ones(nb, dtype=np.int64)
        pose_of[poses] = np.arange(nc)
        lm_all_of = -np.ones(nb, dtype=np.int64)
        lm_all_of[lms_all] = np.arange(lms_all.size)
        mine_mask = np.zeros(nb, dtype=bool)
        mine_mask[lms_all[np.arange(lms_all.size) % world == rank]] = True
        self.lms = np.flatnonzero(mine_mask)
        lm_of = -np.ones(nb, dtype=np.int64)
        lm_of[self.lms] = np.arange(self.lms.size)

        r, c = lam.row_idx, lam.col_idx
        off = r != c
        assert not np.any(off & is_e[r] & is_e[c]), "the eliminated part must be block diagonal"
        # A: pose-pose blocks (upper, i1 <= i2 since the poses keep the block order)
        pa = np.flatnonzero(~is_e[r] & ~is_e[c])
        A_i1, A_i2 = pose_of[r[pa]], pose_of[c[pa]]
        A_blk = _blocks(lam, pa, dp, dp) if pa.size else np.zeros((0, dp, dp))
        self.has_A = np.zeros((nc, nc), dtype=bool)
        self.has_A[A_i1, A_i2] = True
        # observations of ALL landmarks (pattern) and of this shard's (values)
        po = np.flatnonzero(off & (is_e[r] != is_e[c]))
        pose_side = np.where(is_e[r[po]], c[po], r[po])
        lm_side = np.where(is_e[r[po]], r[po], c[po])
        ob_pose_all = pose_of[pose_side]
        ob_lm_all = lm_all_of[lm_side]
        self.k_all = self._pair_counts(nc, ob_lm_all, ob_pose_all, lms_all.size)
        sel = mine_mask[lm_side]
        po, pose_side, lm_side = po[sel], pose_side[sel], lm_side[sel]
        order = np.lexsort((pose_of[pose_side], lm_of[lm_side]))
        po, pose_side, lm_side = po[order], pose_side[order], lm_side[order]
        self.obs_pose = pose_of[pose_side]
        self.obs_lm = lm_of[lm_side]
        # B (dp x dl): the stored block (pose row, landmark column), or the transpose of (landmark row, pose column)
        B = np.empty((po.size, dp, dl))
        st = ~is_e[r[po]]
        if st.any():
            B[st] = _blocks(lam, po[st], dp, dl)
        if (~st).any():
            B[~st] = _blocks(lam, po[~st], dl, dp).transpose(0, 2, 1)
        self.obs_B = B
        nl = self.lms.size
        self.lm_ptr = np.zeros(nl + 1, dtype=np.int64)
        np.cumsum(np.bincount(self.obs_lm, minlength=nl), out=self.lm_ptr[1:])
        pdiag = lam.col_ptr[self.lms + 1] - 1
        assert np.all(lam.row_idx[pdiag] == self.lms), "every landmark needs its diagonal block"
        C = _blocks(lam, pdiag, dl, dl)
        C = np.triu(C) + np.triu(C, 1).transpose(0, 2, 1)   # (the upper triangle is what the solver reads)
        self.C = C
        self.Cinv = _inv_batched(C) if nl else np.zeros((0, dl, dl), dtype=LD)

        # ---- accumulation
        S = np.zeros((n_red, n_red), dtype=LD)
        M = np.zeros((n_red, n_red), dtype=LD)
        rhs = np.zeros(n_red, dtype=LD)
        Mrhs = np.zeros(n_red, dtype=LD)
        if rank == 0:
            for b, i1, i2 in zip(A_blk, A_i1, A_i2):
                S[i1 * dp:(i1 + 1) * dp, i2 * dp:(i2 + 1) * dp] += b
                M[i1 * dp:(i1 + 1) * dp, i2 * dp:(i2 + 1) * dp] += np.abs(b)
            pidx = np.concatenate([np.arange(lam.base[b], lam.base[b + 1]) for b in poses]) if nc else np.zeros(0, int)
            rhs += eta[pidx]
            Mrhs += np.abs(eta[pidx])
        # (the A blocks sit in the upper triangle; the products below fill both triangles: mirror A first)
        S = np.triu(S) + np.triu(S, 1).T
        M = np.triu(M) + np.triu(M, 1).T
        Bl = B.astype(LD)
        Ci = self.Cinv[self.obs_lm] if B.shape[0] else np.zeros((0, dl, dl), dtype=LD)
        Wo = np.matmul(Bl, Ci)                       # B C^-1 per observation
        Wa = np.matmul(np.abs(Bl), np.abs(Ci))
        eta_l = np.empty((B.shape[0], dl), dtype=LD)
        if B.shape[0]:
            lb = lam.base[self.lms][self.obs_lm]
            eta_l[:] = eta[lb[:, None] + np.arange(dl)[None, :]]
        np.subtract.at(rhs.reshape(nc, dp), self.obs_pose, np.einsum("ord,od->or", Wo, eta_l))
        np.add.at(Mrhs.reshape(nc, dp), self.obs_pose, np.einsum("ord,od->or", Wa, np.abs(eta_l)))
        self.obs_count = np.bincount(self.obs_pose, minlength=nc)
        cnt = np.diff(self.lm_ptr)
        rr = np.arange(dp)
        for k in np.unique(cnt[cnt > 0]):   # landmarks of equal track length k together: (n, k, k, dp, dp) products
            ls = np.flatnonzero(cnt == k)
            for l0 in range(0, ls.size, max(1, 200000 // (k * k))):
                lsel = ls[l0:l0 + max(1, 200000 // (k * k))]
                idx = self.lm_ptr[lsel][:, None] + np.arange(k)[None, :]
                P = np.einsum("nard,nbcd->nabrc", Wo[idx], Bl[idx])
                Pm = np.einsum("nard,nbcd->nabrc", Wa[idx], np.abs(Bl[idx]))
                pk = self.obs_pose[idx]
                row = (pk[:, :, None, None, None] * dp + rr[None, None, None, :, None])
                col = (pk[:, None, :, None, None] * dp + rr[None, None, None, None, :])
                flat = (row * n_red + col).ravel()
                np.subtract.at(S.reshape(-1), flat, P.ravel())
                np.add.at(M.reshape(-1), flat, Pm.ravel())
        self.S, self.M, self.rhs, self.Mrhs = S, M, rhs, Mrhs
        self.k = self._pair_counts(nc, self.obs_lm, self.obs_pose, nl)
        up = np.triu(self.k_all > 0) | self.has_A
        i1, i2 = np.nonzero(up)
        o = np.lexsort((i1, i2))
        self.pattern = list(zip(i1[o].tolist(), i2[o].tolist()))

    @staticmethod
    def _pair_counts(nc, ob_lm, ob_pose, nl):
        """k[i, j] = number of landmarks observed by both poses i and j (symmetric; k[i, i] = observations of i)"""
        k = np.zeros((nc, nc), dtype=np.int64)
        if ob_lm.size == 0:
            return k
        o = np.lexsort((ob_pose, ob_lm))
        ob_lm, ob_pose = ob_lm[o], ob_pose[o]
        ptr = np.zeros(nl + 1, dtype=np.int64)
        np.cumsum(np.bincount(ob_lm, minlength=nl), out=ptr[1:])
        cnt = np.diff(ptr)
        for t in np.unique(cnt[cnt > 0]):
            ls = np.flatnonzero(cnt == t)
            pk = ob_pose[ptr[ls][:, None] + np.arange(t)[None, :]]
            np.add.at(k, (np.repeat(pk, t, axis=1).ravel(), np.tile(pk, (1, t)).ravel()), 1)
        return k

    # ---- the library's layouts -----------------------------------------------------------------------------------
    def _elem_k(self):
        """per element of S: the pair count of its block (this shard's)"""
        dp = self.dp
        return np.repeat(np.repeat(self.k, dp, axis=0), dp, axis=1)

    def dense_layout(self, ld):
        """(value, magnitude, pair count, covered) as flat arrays of the dense buffer: ld x ld column-major, S in the upper
        blocks of the pattern, rhs in column n_red; covered = the entries the library writes (the rest must be 0.0)"""
        n, dp = self.n_red, self.dp
        val = np.zeros((ld, ld), dtype=LD)
        mag = np.zeros((ld, ld), dtype=LD)
        kk = np.zeros((ld, ld), dtype=np.int64)
        cov = np.zeros((ld, ld), dtype=bool)
        ek = self._elem_k()
        for i1, i2 in self.pattern:
            s1, s2 = slice(i1 * dp, (i1 + 1) * dp), slice(i2 * dp, (i2 + 1) * dp)
            cov[s1, s2] = True
        val[:n, :n][cov[:n, :n]] = self.S[cov[:n, :n]]
        mag[:n, :n][cov[:n, :n]] = self.M[cov[:n, :n]]
        kk[:n, :n] = np.where(cov[:n, :n], ek, 0)
        val[:n, n], mag[:n, n], kk[:n, n], cov[:n, n] = self.rhs, self.Mrhs, np.repeat(self.obs_count, dp), True
        # column-major flat: element (r, c) at r + c ld  ->  transpose of the row-major image
        return val.T.ravel(), mag.T.ravel(), kk.T.ravel(), cov.T.ravel()

    def sparse_layout(self):
        """(value, magnitude, pair count) of the sparse buffer: the pattern's blocks (column i2, rows ascending), each
        dp x dp column-major, then the n_red rhs"""
        dp = self.dp
        nblk = len(self.pattern)
        i1 = np.array([p[0] for p in self.pattern], dtype=np.int64)
        i2 = np.array([p[1] for p in self.pattern], dtype=np.int64)
        e = np.arange(dp * dp)
        rows = (i1[:, None] * dp + (e % dp)[None, :]).ravel()
        cols = (i2[:, None] * dp + (e // dp)[None, :]).ravel()
        val = np.concatenate([self.S[rows, cols], self.rhs]) if nblk else self.rhs.copy()
        mag = np.concatenate([self.M[rows, cols], self.Mrhs]) if nblk else self.Mrhs.copy()
        kk = np.concatenate([np.repeat(self.k[i1, i2], dp * dp), np.repeat(self.obs_count, dp)])
        return val, mag, kk

    def bound(self, mag, kk, factor=4.0):
        return factor * (kk + 8 * self.dl) * EPS * mag.astype(np.float64)

    def compact(self, dense=True, sparse=True):
        """keep only what the checks read: the library's dense and/or sparse layout (covered values in longdouble, their
        bounds) and, for the whole system (world 1), the refined pose solution with cond(S); then drop the dense
        n_red x n_red S and M"""
        self.layouts = {}
        if dense:
            ld = dense_ld(self.n_red)
            val, mag, kk, cov = self.dense_layout(ld)
            self.layouts["dense"] = (ld, val[cov], self.bound(mag[cov], kk[cov]), cov)
        if sparse:
            val, mag, kk = self.sparse_layout()
            self.layouts["sparse"] = (val, self.bound(mag, kk))
        if self.world == 1:
            self.pose_solution()
        del self.S, self.M
        return self

    def pose_solution(self):
        """(refined x_c = S^-1 rhs, cond(S)), computed once"""
        if not hasattr(self, "x_c_ref"):
            self.x_c_ref = self.solve_poses()
            ev = np.linalg.eigvalsh(self.S.astype(np.float64))
            self.cond_S = float(ev[-1] / ev[0])
        return self.x_c_ref, self.cond_S

    def solve_poses(self, iters=3):
        """x_c = S^-1 rhs: float64 factorization, residuals in longdouble (iterative refinement to ~cond eps^2)"""
        Sd = self.S.astype(np.float64)
        L = np.linalg.cholesky(Sd)
        x = np.zeros(self.n_red, dtype=LD)
        for _ in range(iters + 1):
            res = self.rhs - self.S @ x
            y = np.linalg.solve(L, res.astype(np.float64))
            x = x + np.linalg.solve(L.T, y).astype(LD)
        return x

    def backsubstitute(self, lam, eta, x_c):
        """per landmark of the shard: x_l = C_l^-1 (eta_l - sum B^T x_c) in longdouble, and its magnitude
        |C_l^-1| (|eta_l| + sum |B|^T |x_c|) and observation count -- arrays (nl, dl), (nl, dl), (nl,)"""
        dp, dl = self.dp, self.dl
        nl = self.lms.size
        xc = np.asarray(x_c, dtype=LD).reshape(-1, dp)
        el = eta[lam.base[self.lms][:, None] + np.arange(dl)[None, :]].astype(LD) if nl else np.zeros((0, dl), LD)
        t = el.copy()
        tm = np.abs(el)
        Bl = self.obs_B.astype(LD)
        np.subtract.at(t, self.obs_lm, np.einsum("ord,or->od", Bl, xc[self.obs_pose]))
        np.add.at(tm, self.obs_lm, np.einsum("ord,or->od", np.abs(Bl), np.abs(xc[self.obs_pose])))
        xl = np.einsum("lde,le->ld", self.Cinv, t)
        ml = np.einsum("lde,le->ld", np.abs(self.Cinv), tm)
        return xl, ml, np.diff(self.lm_ptr)


def pose_index(lam, blocks):
    return np.concatenate([np.arange(lam.base[b], lam.base[b + 1]) for b in blocks]) if len(blocks) else np.zeros(0, np.int64)


def dense_ld(n_red):
    """leading dimension of the library's dense S: whole 128-column tiles, at least one padding column (the rhs)"""
    return ((n_red + 1 + 127) // 128) * 128


def _within(got, val, bnd, what):
    """|got - val| <= bnd elementwise (exact where the bound is 0; a NaN or an infinity anywhere fails); returns the
    largest ratio error / bound"""
    err = np.abs(got.astype(LD) - val).astype(np.float64)
    bad = np.flatnonzero(~(err <= bnd))
    assert bad.size == 0, "%s: %d entries outside the bound, first at %d: got %r, ref %r, bound %.3e" % (
        what, bad.size, bad[0], got[bad[0]], float(val[bad[0]]), bnd[bad[0]])
    pos = bnd > 0
    return float((err[pos] / bnd[pos]).max()) if pos.any() else 0.0


def check_schur_buffer(R, buf, sparse, ld=0):
    """the library's S | rhs buffer (dense: ld x ld column-major, sparse: block values | rhs) against the reference:
    every entry the library writes within 4 (k + 8 dl) eps M, every other entry of the dense buffer exactly 0.0.
    Returns the largest ratio of error to bound."""
    layouts = getattr(R, "layouts", {})
    if sparse:
        if "sparse" in layouts:
            val, bnd = layouts["sparse"]
        else:
            val, mag, kk = R.sparse_layout()
            bnd = R.bound(mag, kk)
        assert buf.size == val.size, (buf.size, val.size)
        return _within(buf, val, bnd, "sparse S | rhs")
    assert ld == dense_ld(R.n_red), (ld, R.n_red)
    if "dense" in layouts:
        _, val_c, bnd_c, cov = layouts["dense"]
    else:
        val, mag, kk, cov = R.dense_layout(ld)
        val_c, bnd_c = val[cov], R.bound(mag[cov], kk[cov])
    assert buf.size == ld * ld, (buf.size, ld)
    out = np.flatnonzero(~cov & (buf != 0.0))   # (a NaN is != 0.0 too)
    assert out.size == 0, "dense S: %d entries outside the upper blocks and the rhs column are not 0.0 (first at %d: %r)" % (
        out.size, out[0], buf[out[0]])
    return _within(buf[cov], val_c, bnd_c, "dense S | rhs")


def check_solution(R, lam, eta, x, res_tol=1e-11):
    """x of the whole system (unsharded reference): every landmark's part against C_l^-1 (eta_l - sum B^T x_c) with the
    library's own pose part x_c (independent of the conditioning of S), the pose part against a refined longdouble solve
    of S_ref, and the residual of the full system. Returns (largest landmark error / bound, pose part relative error /
    bound)."""
    dp, dl = R.dp, R.dl
    xc = x[pose_index(lam, R.poses)]
    xl_ref, ml, kl = R.backsubstitute(lam, eta, xc)
    xl = x[lam.base[R.lms][:, None] + np.arange(dl)[None, :]] if R.lms.size else np.zeros((0, dl))
    cond_l = np.linalg.cond(R.C) if R.lms.size else np.zeros(0)
    bnd = 4 * (kl[:, None] + 8 * dl) * EPS * np.maximum(1.0, cond_l)[:, None] * ml.astype(np.float64)
    r_l = _within(xl.ravel(), xl_ref.ravel(), bnd.ravel(), "landmark part of x")
    x_c_ref, cond_S = R.pose_solution()
    e_c = float(np.linalg.norm((xc - x_c_ref).astype(np.float64)) / np.linalg.norm(x_c_ref.astype(np.float64)))
    b_c = 64 * cond_S * EPS
    assert e_c <= b_c, ("pose part of x", e_c, b_c)   # (fails on NaN too)
    res = np.linalg.norm(lam.matvec(x) - eta) / np.linalg.norm(eta)
    assert res < res_tol, ("residual", res)
    return r_l, e_c / b_c


def schur_ref(lam, eta, elim, rank=0, world=1):
    return SchurRef(lam, eta, elim, rank, world)


def guided_elim(lam):
    """the eliminated set of the guided Schur modes: every block of the smaller width"""
    return np.flatnonzero(lam.dim == lam.dim.min())
