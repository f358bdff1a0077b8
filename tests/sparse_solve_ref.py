"""Reference machinery of the solve-again tests of the SPARSE path (test infrastructure, numpy / scipy on the host only).

Systems: the designed fixtures of tests/sparse_fixtures.py (every front class, chosen) and the two small pose graphs
se2_small / se3_small assembled with damping POSE_DAMPING, as tests/sparse_fronts_child.py assembles them.

refined_columns(name, B): for a designed fixture, per connected component a float64 Cholesky solve of Fixture.dense
refined with the residual in longdouble -- sparse_fixtures.reference, column by column with the factor computed once; for
a pose graph tests/solve_again_ref.py's refiner (parity.refined_solution with its LU kept). covariance_ref assembles
E^T Lambda^-1 E from the refined unit columns. Everything is cached per system: the GPU tests share one reference and
never change it."""
import numpy as np

import solve_again_ref as sar
import sparse_fixtures as sf

POSE = ("se2_small", "se3_small")
POSE_DAMPING = 50.0     # cond(Lambda) 2.5e3 / 1.1e4 (tests/test_sparse_solve_ref_host.py measures it): below sar.COND_MAX
K_MAX = 17
K_WIDE = {"tree_hi": 129}   # classes 0..4 in one tree; two passes of 128 columns
PASSES = 3

_CACHE = {}


def fixture(name):
    if ("fx", name) not in _CACHE:
        _CACHE[("fx", name)] = sf.build(name)
    return _CACHE[("fx", name)]


def problem(name):
    """(lam, eta) of a designed fixture or a damped pose graph"""
    if ("p", name) not in _CACHE:
        if name in POSE:
            from slam_plus_plus_amd import synth
            from oracle import spp_oracle as orc
            _CACHE[("p", name)] = orc.assemble(synth.make(name), damping=POSE_DAMPING)
        else:
            fx = fixture(name)
            _CACHE[("p", name)] = (fx.lam, fx.eta)
    return _CACHE[("p", name)]


class _ComponentRefiner:
    """sparse_fixtures.reference with the Cholesky factors and the longdouble images of the components kept"""

    def __init__(self, fx):
        import scipy.linalg as sla
        self.fx = fx
        self.cf = [sla.cho_factor(L) for L in fx.dense]
        self.Ll = [L.astype(np.longdouble) for L in fx.dense]

    def solve(self, eta, passes=PASSES):
        import scipy.linalg as sla
        x = np.zeros(self.fx.lam.n)
        for s, cf, Ll in zip(self.fx.comp_scalars, self.cf, self.Ll):
            b = eta[s].astype(np.longdouble)
            xc = sla.cho_solve(cf, eta[s]).astype(np.longdouble)
            for _ in range(passes):
                dx = sla.cho_solve(cf, (b - Ll @ xc).astype(np.float64)).astype(np.longdouble)
                xc = xc + dx
            x[s] = xc.astype(np.float64)
        return x


def refiner(name):
    if ("rf", name) not in _CACHE:
        _CACHE[("rf", name)] = sar._Refiner(problem(name)[0]) if name in POSE else _ComponentRefiner(fixture(name))
    return _CACHE[("rf", name)]


def refined_columns(name, B):
    rf = refiner(name)
    return np.stack([rf.solve(np.ascontiguousarray(B[:, j])) for j in range(B.shape[1])], axis=1)


def leaf_and_separator_rows(name):
    """a scalar row inside a leaf front and one inside a separator front (pose graphs: the middle and the last pose)"""
    lam = problem(name)[0]
    if name in POSE:
        return int(lam.base[lam.nb // 2] + 1), int(lam.base[lam.nb - 1] + lam.dim[lam.nb - 1] - 1)
    fx = fixture(name)
    leaf = [g for g in fx.cliques if g["role"] == "leaf"][0]["blocks"]
    sep = max((g for g in fx.cliques if g["role"] == "separator"), key=lambda g: g["width"])["blocks"]
    vl, vs = int(leaf[leaf.size // 2]), int(sep[sep.size // 3])
    return int(lam.base[vl] + lam.dim[vl] - 1), int(lam.base[vs])


def rhs_columns(name):
    """the right-hand sides of a system, built as solve_again_ref.rhs_columns builds them: [eta, random, e of a leaf row,
    e of a separator row, random ...], K_MAX columns (K_WIDE: more); the tests with fewer columns take the leading ones"""
    if ("B", name) not in _CACHE:
        lam, eta = problem(name)
        k = K_WIDE.get(name, K_MAX)
        rng = np.random.default_rng(len(name) + 1000 * k)
        B = rng.standard_normal((lam.n, k))
        B[:, 0] = eta
        r_leaf, r_sep = leaf_and_separator_rows(name)
        B[:, 2] = 0.0
        B[r_leaf, 2] = 1.0
        B[:, 3] = 0.0
        B[r_sep, 3] = 1.0
        _CACHE[("B", name)] = B
    return _CACHE[("B", name)]


def rhs_reference(name):
    if ("X", name) not in _CACHE:
        _CACHE[("X", name)] = refined_columns(name, rhs_columns(name))
    return _CACHE[("X", name)]


def covariance_ref(name, vertices):
    """(E^T Lambda^-1 E from refined unit-column solves, the refined columns themselves, the selected rows)"""
    lam = problem(name)[0]
    E, rows = sar.unit_columns(lam, vertices)
    X = refined_columns(name, E)
    return X[rows], X, rows


def condition(name):
    """cond_2 of Lambda: the worst connected component of a designed fixture, the dense Lambda of a pose graph"""
    if ("cond", name) not in _CACHE:
        if name in POSE:
            c = float(np.linalg.cond(problem(name)[0].to_scipy().toarray()))
        else:
            c = max(float(np.linalg.cond(L)) for L in fixture(name).dense)
        _CACHE[("cond", name)] = c
    return _CACHE[("cond", name)]


def marginal_selection(name):
    """the vertices the marginals test selects. Designed: one block of the first leaf, of the widest leaf and of the
    separator, plus a width-1 and a width-8 block, shuffled. Pose graphs: the first, middle and last pose and two
    adjacent ones."""
    lam = problem(name)[0]
    if name in POSE:
        nb = lam.nb
        return [0, nb // 2, nb - 1, nb // 3, nb // 3 + 1]
    fx = fixture(name)
    leaves = [g for g in fx.cliques if g["role"] == "leaf"]
    sep = max((g for g in fx.cliques if g["role"] == "separator"), key=lambda g: g["width"])
    widest = max(leaves, key=lambda g: g["width"])
    sel = [int(leaves[0]["blocks"][0]), int(widest["blocks"][-1]), int(sep["blocks"][sep["blocks"].size // 2])]
    for d in (1, 8):
        sel.append(next(int(v) for v in np.flatnonzero(lam.dim == d) if int(v) not in sel))
    rng = np.random.default_rng(len(name))
    return [sel[i] for i in rng.permutation(len(sel))]
