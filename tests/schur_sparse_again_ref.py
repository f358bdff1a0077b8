"""Fixture and reference of the tests of the kept factor of a sparse reduced system (test infrastructure, numpy / scipy on
the host only): spp_schur_sparse_solve_device, spp_schur_sparse_marginals_device, spp_schur_sparse_sigma_device.

The fixtures of tests/schur_sigma_ref.py are chains, loops and stars of few cameras per landmark: analyzed in
MODE_SCHUR_SPARSE their reduced systems give fronts of classes 0 - 2 only. cliques63 adds the two larger classes, each as
a parent and as a child (classes go by padded front height: <= 32 / 64 / 128 / SPP_MID_FRONT_MAX = 320 / above). The
library orders the cameras by minimum degree, so what many cameras see together is eliminated last:

  A    60 six-wide cameras, three landmarks seen by all of them: 360 reduced rows, the root front, class 4
  G    25 cameras, three landmarks seen by all of them and one more seen by them and 5 cameras of A: 150 pivot rows over 30
       update rows, class 3, a child of A's front
  M    32 cameras and a landmark seen by them and 23 cameras of A: 192 pivot rows over 138 update rows, class 4, a child of
       A's front
  L    6 cameras and a landmark seen by them and 4 cameras of G: a child of G's front
(the library merges a child into its parent when that buys few explicit zeros: M and L are wide and loosely tied enough to
stay fronts of their own)
  H    a chain of 6 cameras, consecutive ones tied by a landmark each, its head tied to 3 cameras of A
  P    3 single cameras, each tied to two cameras of A by a landmark: 6 pivot rows over 12 update rows, class 0, eliminated
       long before their parent (a front next to its parent in the order and at most 32 wide with it is merged into it)

Every camera also sees two landmarks of its own (degree 1), one landmark is seen by nobody, and camera-camera blocks tie
cameras inside A, inside G, across (G, A) and along the chain, one of them two cameras that share no landmark (a block of S's
pattern that A alone gives). 132 cameras, 283 landmarks, n = 1641.
tests/test_gpu_schur_sparse_again.py asserts the classes from Context.sparse_fronts().

problem(name) serves this fixture and every fixture of tests/schur_sigma_ref.py; seeding solve_again_ref's cache with
cliques63 makes that module's and schur_sigma_ref's machinery (parts, reference, refiner, rhs_columns ...) work on it by
name. Everything is cached: the GPU tests share one reference and never change it."""
import numpy as np

import schur_fixtures as fx
import schur_sigma_ref as ssg
import solve_again_ref as sar

NEW = "cliques63"
FIXTURES = ssg.FIXTURES + [NEW]
FULL = ssg.FULL + [NEW]            # every stored block is also compared with the solve route on all n unit columns
SCHEDULED = ["loop63", "chain73", NEW]
N_A, N_G, N_M, N_L, N_H, N_P = 60, 25, 32, 6, 6, 3
A_OF_G, A_OF_M, G_OF_L, A_OF_H = 5, 23, 4, 3
SEED = 6334


def cliques63():
    a0, g0 = 0, N_A
    m0, l0, h0 = g0 + N_G, g0 + N_G + N_M, g0 + N_G + N_M + N_L
    p0 = h0 + N_H
    nc = p0 + N_P
    A, G = list(range(a0, a0 + N_A)), list(range(g0, g0 + N_G))
    M, L, H = list(range(m0, m0 + N_M)), list(range(l0, l0 + N_L)), list(range(h0, h0 + N_H))
    tracks = [A, A, A, G, G, G,
              G + A[10:10 + A_OF_G],                 # G hangs on 5 cameras of A
              M + A[N_A - A_OF_M:],                  # M on 23
              L + G[3:3 + G_OF_L],                   # L on 4 cameras of G
              [H[0]] + A[:A_OF_H]]                   # the chain's head on 3
    tracks += [[H[q], H[q + 1]] for q in range(N_H - 1)]
    tracks += [[p0 + q, A[30 + 2 * q], A[31 + 2 * q]] for q in range(N_P)]
    tracks += [[c] for c in range(nc) for _ in range(2)]
    obs, lm = [], 0
    for t in tracks:
        obs += [(c, lm) for c in t]
        lm += 1
    lm += 1                                          # a landmark nobody sees: C is the damping alone
    a_edges = [(A[1], A[7]), (A[20], A[59]), (G[0], G[24]), (G[2], A[12]), (H[1], H[2]), (H[1], H[3]), (H[4], H[5])]
    return fx._guided(nc, lm, 6, 3, obs, a_edges, SEED)


def problem(name):
    if name == NEW and ("p", NEW) not in sar._CACHE:
        sar._CACHE[("p", NEW)] = cliques63()
    lam_eta = ssg.problem(name)
    sar._CACHE.setdefault(("p", name), lam_eta)      # (ba_interleaved: schur_sigma_ref keeps it in a cache of its own)
    return lam_eta


def marginal_vertices(name):
    """five vertices: the first, middle and last camera, the first and the last landmark"""
    problem(name)
    P = ssg.parts(name)
    return np.array([P.cams[0], P.cams[P.cams.size // 2], P.cams[-1], P.lms[0], P.lms[-1]], dtype=np.int64)


def reference(name):
    """Sigma on the pattern of Lambda, NVALS float64: schur_sigma_ref's formulas on the refined inverse of S"""
    problem(name)
    return ssg.reference(name)
