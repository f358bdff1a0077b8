"""Edge fixtures of the Schur stage for 7-wide cameras (Sim(3)) and 3-wide points, built by the generator of
tests/schur_fixtures.py, unchanged (test infrastructure, numpy only).

  edges73          320 cameras, n_red = 2240 = 17.5 tiles of 128: cameras straddle tile boundaries (7 does not divide 128),
                   the rhs column lies inside the last tile. The pair-count spread of edges63 (1, 63, 64, 65, 128, 2047,
                   2048, 2049 and 4100 pairs), A-only blocks, a camera without observations, the 256-observer track.
  edges73_aligned  128 cameras, n_red = 896 = 7 * 128: the rhs column is the first padding column; no 256-observer track
  loop73, chain73  a closed loop whose camera order is accepted and an open chain with unlisted tiles (fx.ring)
  tiny_shards73    4 cameras, 2 landmarks: a landmark shard can be empty"""
import schur_fixtures as fx

ALIGNED_SEED = 731   # (largest landmark condition 5.2; tests/test_schur_fixtures_73_host.py asserts the limit)


def edges73():
    return fx._edges_guided(320, 7, 3, 73)


def edges73_aligned():
    return fx._edges_guided(128, 7, 3, ALIGNED_SEED, track256=False)


LOOP73_SPLIT = (137, 142)


def loop73():
    """330 cameras in a loop (fx.ring: co-visibility +-12 cameras), n_red = 2310, 19 tile rows. The arc length of the
    camera order is 128 / gcd(128, 7) = 128 cameras; the order is accepted, camera-camera blocks occur in both senses and
    the split pair (137 in the separator, 142 in arc B) is reversed (tests/test_schur_fixtures_73_host.py asserts it)"""
    return fx.ring(330, 7, 3, half=12, seed=5, split=LOOP73_SPLIT)


def chain73():
    """an open chain of 92 cameras (co-visibility +-4), n_red = 644, 6 tile rows: 128 t / 7 is whole for no t = 1..5, a
    camera straddles every tile boundary; the natural order is kept and tiles stay unlisted"""
    return fx.ring(92, 7, 3, half=4, seed=92, wrap=False)


def tiny_shards73():
    return fx._tiny_shards(7, 47)


ALL = {"edges73": edges73, "edges73_aligned": edges73_aligned}
SHAPES = {"loop73": loop73, "chain73": chain73, "tiny_shards73": tiny_shards73}   # (no pair-count spread)


def make(name):
    return (ALL[name] if name in ALL else SHAPES[name])()


def make_any(name):
    """a fixture of this file or of tests/schur_fixtures.py"""
    return make(name) if name in ALL or name in SHAPES else fx.make(name)
