"""Designed systems for the sparse path (test infrastructure, numpy only): block graphs whose frontal matrices can be
chosen, unlike those of the workload pose graphs.

Structures. Every system is a union of CLIQUES of the block graph:
  * a clique forest: disjoint complete block graphs. A clique is one supernode under any elimination order, a root with
    h = w + 1 (the + 1 is the right-hand-side slot every front carries), so its scalar width w alone picks the size class
    (hp16 = roundup16(w) + 16), the padding and the backward kernel;
  * clique trees: a separator clique S and leaf cliques A_i, each leaf fully connected to a strict subset S_i of S that is
    drawn at random over S's blocks (gaps: the leaf's rows are not contiguous in the parent); a chain adds a third level.
    With the amalgamation switches at zero only zero-fill merges happen and a leaf stays a front of its own:
    w = |A_i|, h = |A_i| + |S_i| + 1.
Block widths are ragged (dealt from shuffled decks of 1..8, narrowed to a range for some cliques, the last block of a
clique takes the remainder) and the vertex ids are shuffled, so both orientations of a stored block occur after the library's permutation.

Values. Lambda = I + sum over the cliques K of s_K J_K^T J_K, J_K a ROWS x |K| matrix over ALL scalars of the clique and
s_K = s / |K|, s per connected component such that cond_2 <= COND (lambda_min >= 1, lambda_max = COND). This is what
_spd_blocks of test_gpu_edge_cases.py does for a two-block clique. Two things differ, both for the sake of the sensitivity
that test_sparse_fixtures_host.py measures (every stored block must move x by more than the accuracy bound of the GPU
test when it changes):
  * one J per clique, not per block PAIR: summed per pair a large clique is strongly diagonally dominant (every diagonal
    block collects m - 1 terms, every other block one) and a lost block of a 1024-wide clique moves x by less than 1e-12;
  * the first row of J has entries in [1, 2], the other rows are Gaussian with deviation NOISE: a purely Gaussian J makes
    a 1 x 1 block a sum of products of either sign, as close to zero as chance has it -- and a block that is almost zero
    cannot be missed. Every block is s_K (u_i u_j^T + noise of a quarter of that) and no two entries are equal.
The right-hand side is Lambda x0 with |x0| in [1, 2]."""
import numpy as np

from slam_plus_plus_amd.blockcsc import structure_from_pairs

ROWS = 8       # rows of a clique's J: one of entries in [1, 2], the others Gaussian of deviation NOISE
NOISE = 0.3
COND = 80.0    # cond_2 of every connected component (by construction; the host test measures it)

FOREST_WIDTHS = {
    "forest_a": [1, 15, 16, 17, 48, 49, 112, 113, 191, 192],
    "forest_b": [304, 305, 384, 385],
    "forest_c": [624, 625, 1023, 1024],
}
FOREST_TREE = (20, (1, 8), [(0, 6, (1, 8)), (36, 9, "each"), (0, 11, (1, 8))])   # the one small tree every forest carries

# Trees: per connected component (separator width, its block widths, [(leaf width, width of S_i, leaf block widths) ...]);
# a leaf width of 0: ONE block. The orderings count BLOCKS: a leaf (|A_i| + |S_i| - 1 neighbours per block) is eliminated
# before any block of its separator (at least |S| - 1 neighbours) as long as |A_i| + |S_i| < |S| in blocks, whatever the
# scalar widths -- so the wide leaves under narrow separators are made of wide blocks and those separators of narrow ones.
# The fronts are then the leaves (w = |A_i|, h = |A_i| + |S_i| + 1) and the separator (w = |S|, a root).
ANY, NARROW, WIDE = (1, 8), (1, 1), (7, 8)
EACH = "each"   # a leaf of eight blocks, every width 1..8 once (36 scalars): every fixture has every block width
TREES = {
    # parents of class 0 and 1 with children of classes 0..2
    "small_trees": [(12, NARROW, [(0, 5, ANY), (0, 8, ANY), (5, 4, ANY)]),
                    (40, (1, 2), [(36, 8, EACH), (30, 20, WIDE), (70, 20, WIDE), (0, 12, ANY)])],
    # 64 one-block leaves under one separator (class 2), S_i between 3 and 30 wide
    "star": [(60, ANY, [(0, (3, 8, 14, 22, 30)[i % 5], ANY) for i in range(64)])],
    # children of classes 0..2, 3 and 4 under a parent of class 2, 3 and 4 (with the default SPP_MID_FRONT_MAX)
    "tree_lo": [(112, NARROW, [(6, 20, ANY), (36, 40, EACH), (70, 40, ANY), (150, 40, WIDE), (300, 40, WIDE)])],
    "tree_mid": [(200, (1, 2), [(6, 20, ANY), (36, 20, EACH), (150, 100, WIDE), (300, 100, WIDE)])],
    "tree_hi": [(400, (1, 4), [(6, 30, ANY), (36, 30, EACH), (150, 120, WIDE), (280, 150, WIDE)])],
}
# three levels: root R, a middle clique M connected to a subset of R, small leaves connected to subsets of M
CHAIN = dict(R=150, R_blocks=(1, 2), M=100, M_blocks=WIDE, R_M=60,
             leaves=[(0, 10, ANY), (0, 20, ANY), (6, 12, ANY), (10, 25, ANY), (3, 7, ANY), (0, 30, ANY), (36, 10, EACH)])

NAMES = list(FOREST_WIDTHS) + list(TREES) + ["chain"]
TREE_NAMES = list(TREES) + ["chain"]

LEAF, SEP = 0, 1
KINDS = ("leaf", "separator", "coupling")


class Fixture:
    """name; lam (BlockCSC with values), eta; comp_blocks[c]: block ids of connected component c (ascending);
    comp_scalars[c]: their scalar indices; dense[c]: the component's dense Lambda; cliques: dicts(comp, role, width,
    blocks) of the designed cliques (leaf / separator groups); block_kind[p]: index into KINDS of stored block p"""


class _Deck:
    def __init__(self, rng):
        self.rng, self.left = rng, []

    def deal(self):
        if not self.left:
            self.left = list(self.rng.permutation(np.arange(1, 9)))
        return int(self.left.pop())


class _Builder:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.deck = _Deck(self.rng)
        self.dim, self.role, self.comp = [], [], []
        self.groups, self.cliques = [], []

    def group(self, width, role, comp, blocks=ANY):
        """new blocks of ragged widths within `blocks` summing to `width` (0: one block)"""
        ids, left = [], width
        each = list(self.rng.permutation(np.arange(1, 9))) if blocks == EACH else None
        assert each is None or width == 36
        while True:
            d = int(each.pop()) if each else blocks[0] + (self.deck.deal() - 1) % (blocks[1] - blocks[0] + 1)
            if width > 0:
                d = min(d, left)
            ids.append(len(self.dim))
            self.dim.append(d)
            self.role.append(role)
            self.comp.append(comp)
            left -= d
            if width <= 0 or left == 0:
                break
        ids = np.array(ids, dtype=np.int64)
        self.groups.append(dict(comp=comp, role=("leaf", "separator")[role], width=int(sum(self.dim[i] for i in ids)), blocks=ids))
        return ids

    def subset(self, blocks, width):
        """a strict random subset of `blocks` of about `width` scalars (random over the blocks: gaps)"""
        pick, tot = [], 0
        for b in self.rng.permutation(blocks):
            if tot >= width or len(pick) == len(blocks) - 1:
                break
            pick.append(int(b))
            tot += self.dim[b]
        return np.array(sorted(pick), dtype=np.int64)

    def clique(self, *parts):
        self.cliques.append(np.concatenate(parts))

    def tree(self, comp, sep_width, sep_blocks, leaves):
        S = self.group(sep_width, SEP, comp, sep_blocks)
        self.clique(S)
        for (wl, ws, leaf_blocks) in leaves:
            A = self.group(wl, LEAF, comp, leaf_blocks)
            self.clique(A, self.subset(S, ws))
        return S


def build(name, seed=20240):
    b = _Builder(seed + NAMES.index(name))
    if name in FOREST_WIDTHS:
        for c, w in enumerate(FOREST_WIDTHS[name]):
            b.clique(b.group(w, SEP, c))
        # (a clique alone is one supervariable of the ordering, eliminated in one run of descending ids: ALL its stored
        # blocks arrive transposed. One small tree per forest brings the other orientation: leaf before separator.)
        b.tree(len(FOREST_WIDTHS[name]), *FOREST_TREE)
    elif name in TREES:
        for c, (ws, sep_blocks, leaves) in enumerate(TREES[name]):
            b.tree(c, ws, sep_blocks, leaves)
    else:
        R = b.group(CHAIN["R"], SEP, 0, CHAIN["R_blocks"])
        b.clique(R)
        M = b.group(CHAIN["M"], SEP, 0, CHAIN["M_blocks"])
        b.clique(M, b.subset(R, CHAIN["R_M"]))
        for (wl, ws, leaf_blocks) in CHAIN["leaves"]:
            b.clique(b.group(wl, LEAF, 0, leaf_blocks), b.subset(M, ws))
    return _finish(name, b)


def _finish(name, b):
    rng = b.rng
    nb = len(b.dim)
    new_id = rng.permutation(nb)                       # shuffled vertex ids: old block v becomes new_id[v]
    dim = np.zeros(nb, dtype=np.int32)
    role = np.zeros(nb, dtype=np.int64)
    comp = np.zeros(nb, dtype=np.int64)
    dim[new_id], role[new_id], comp[new_id] = b.dim, b.role, b.comp
    cliques = [np.sort(new_id[k]) for k in b.cliques]
    rows, cols = [], []
    for k in cliques:
        i, j = np.triu_indices(k.size, 1)
        rows.append(k[i])
        cols.append(k[j])
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    st, _, _ = structure_from_pairs(dim, rows, cols)
    base = st.base
    fx = Fixture()
    fx.name = name
    ncomp = int(comp.max()) + 1
    fx.comp_blocks = [np.flatnonzero(comp == c) for c in range(ncomp)]
    fx.comp_scalars = [np.concatenate([np.arange(base[v], base[v + 1]) for v in blk]) for blk in fx.comp_blocks]
    loc = np.zeros(nb, dtype=np.int64)                 # offset of a block inside its component
    for blk in fx.comp_blocks:
        loc[blk] = np.concatenate([[0], np.cumsum(dim[blk])[:-1]])
    M = [np.zeros((s.size, s.size)) for s in fx.comp_scalars]
    for k in cliques:
        idx = np.concatenate([np.arange(loc[v], loc[v] + dim[v]) for v in k])
        J = np.vstack([rng.uniform(1.0, 2.0, size=(1, idx.size)), NOISE * rng.normal(size=(ROWS - 1, idx.size))])
        M[comp[k[0]]][np.ix_(idx, idx)] += (J.T @ J) / idx.size
    fx.dense = []
    for m in M:
        lmax = float(np.linalg.eigvalsh(m)[-1])
        fx.dense.append(np.eye(m.shape[0]) + ((COND - 1.0) / lmax) * m)
    vals = np.zeros(st.nvals)
    col_idx = st.col_idx
    kind = np.zeros(st.nnzb, dtype=np.int64)
    for p in range(st.nnzb):
        i, j = int(st.row_idx[p]), int(col_idx[p])
        di, dj = int(dim[i]), int(dim[j])
        vals[st.blk_off[p]:st.blk_off[p] + di * dj] = fx.dense[comp[i]][loc[i]:loc[i] + di, loc[j]:loc[j] + dj].ravel(order="F")
        kind[p] = role[i] if role[i] == role[j] else 2
    fx.lam = st.with_vals(vals)
    # right-hand side: Lambda x0 with |x0| in [1, 2] everywhere -- no part of the solution is small, so every block has
    # something to multiply (a random eta leaves the stiff separator rows of x some 50 times smaller than the rest)
    x0 = rng.uniform(1.0, 2.0, size=st.n) * rng.choice([-1.0, 1.0], size=st.n)
    fx.eta = np.zeros(st.n)
    for s, L in zip(fx.comp_scalars, fx.dense):
        fx.eta[s] = L @ x0[s]
    fx.block_kind = kind
    fx.cliques = [dict(g, blocks=np.sort(new_id[g["blocks"]])) for g in b.groups]
    return fx


def reference(fx, passes=3):
    """per connected component: float64 Cholesky solve refined with the residual in longdouble (as parity.refined_solution
    does for the sparse workloads). Returns (x_ref, change): change[c] = relative size of the last pass's correction."""
    import scipy.linalg as sla
    x = np.zeros(fx.lam.n)
    change = []
    for s, L in zip(fx.comp_scalars, fx.dense):
        cf = sla.cho_factor(L)
        Ll = L.astype(np.longdouble)
        b = fx.eta[s].astype(np.longdouble)
        xc = sla.cho_solve(cf, fx.eta[s]).astype(np.longdouble)
        for _ in range(passes):
            dx = sla.cho_solve(cf, (b - Ll @ xc).astype(np.float64)).astype(np.longdouble)
            xc = xc + dx
        change.append(float(np.sqrt((dx * dx).sum() / (xc * xc).sum())))
        x[s] = xc.astype(np.float64)
    return x, change


def lapack_solution(fx):
    """plain float64 Cholesky solve per component (the yardstick the GPU error is printed beside)"""
    import scipy.linalg as sla
    x = np.zeros(fx.lam.n)
    for s, L in zip(fx.comp_scalars, fx.dense):
        x[s] = sla.cho_solve(sla.cho_factor(L), fx.eta[s])
    return x


def component_errors(fx, x, x_ref):
    """relative error of x per connected component"""
    return [float(np.linalg.norm(x[s] - x_ref[s]) / np.linalg.norm(x_ref[s])) for s in fx.comp_scalars]


def diagonal_block(fx, v):
    """index of the stored diagonal block of block column v"""
    return int(fx.lam.col_ptr[v + 1] - 1)


def clique_of_width(fx, width):
    for g in fx.cliques:
        if g["width"] == width:
            return g
    raise KeyError(width)
