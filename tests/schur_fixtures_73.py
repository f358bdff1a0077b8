"""Edge fixtures of the Schur stage for 7-wide cameras (Sim(3)) and 3-wide points, built by the generator of
tests/schur_fixtures.py, unchanged (test infrastructure, numpy only).

  edges73          320 cameras, n_red = 2240 = 17.5 tiles of 128: cameras straddle tile boundaries (7 does not divide 128),
                   the rhs column lies inside the last tile. The pair-count spread of edges63 (1, 63, 64, 65, 128, 2047,
                   2048, 2049 and 4100 pairs), A-only blocks, a camera without observations, the 256-observer track.
  edges73_aligned  128 cameras, n_red = 896 = 7 * 128: the rhs column is the first padding column; no 256-observer track"""
import schur_fixtures as fx

ALIGNED_SEED = 731   # (largest landmark condition 5.2; tests/test_schur_fixtures_73_host.py asserts the limit)


def edges73():
    return fx._edges_guided(320, 7, 3, 73)


def edges73_aligned():
    return fx._edges_guided(128, 7, 3, ALIGNED_SEED, track256=False)


ALL = {"edges73": edges73, "edges73_aligned": edges73_aligned}


def make(name):
    return ALL[name]()
