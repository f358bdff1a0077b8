"""The clear of the solver's own dense S buffer by listed tiles. Invariant: a tile of S outside the filled mask is zero
whenever a factorization starts. The fully masked streamed launch keeps it (a tile without a workgroup is never written),
so the next spp_factor_solve_device clears the listed tiles alone; every other schedule marks the buffer and the next call
clears all of it.

A stale tile can only show where the mask has holes: an open chain of 90 cameras (5 tile rows, tiles (0, 2), (0, 3), (1, 3)
empty), the 300-camera ring of tests/test_gpu_dense_tilemask.py (15 tile rows), and with 7-wide cameras an open chain of
92 (chain73, 6 tile rows), a loop of 330 (loop73, 19 tile rows) and edges73_aligned (7 tile rows). In ONE context values A, values B, then A
again are solved, then a non-positive pivot and B again: each good solve must equal (numpy.array_equal) the solve of a
fresh context on the same values. The children (tests/schur_side_child.py; the switches are read once per process) also
report what each solve cleared (SPP_INFO_S_CLEAR) and which tiles of the S buffer hold anything afterwards.

Not covered: a change of schedule on the solver's S buffer inside one process. The API reaches that buffer through
spp_factor_solve_device alone and the switches are fixed per process, so the fallback schedules run in children of their
own, and spp_dense_posv_masked (a buffer of its own) runs between two streamed solves of one context."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "schur_side_child.py")
SWITCHES = ["SPP_SCHUR_SIDE", "SPP_DENSE_TAIL", "SPP_TAIL_MASK", "SPP_TAIL_ROWS", "SPP_SCHUR_CAM_ORDER"]
# 7-wide cameras (tests/schur_fixtures_73.py): a block straddles two tiles in either direction at other places than a
# 6-wide one does, and a mask that marked one of the two would leave the other uncleared -- and unlisted. In a band
# (chain73, loop73) the symbolic fill lists the second tile anyway; in edges73_aligned (7 tile rows, S next to block
# diagonal) the upper right corner of the diagonal block of camera 18 (rows 126..132) is all that tile (0, 1) holds
TILE_ROWS = {"chain90": 5, "ba_ring300": 15, "chain73": 6, "loop73": 19, "edges73_aligned": 7}


def _run(name, env_extra, **opt):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(env_extra)
    r = subprocess.run([sys.executable, CHILD, "clear", name, json.dumps(opt)], env=env, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, "%s %s: exit %d\n%s%s" % (name, env_extra, r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    print(name, env_extra, "cleared", res["clear"], "streamed", res["streamed"], "side", res["side"], res["equal"])
    return res


def _all_equal(res):
    for tag, ok in res["equal"]:
        assert ok, "solve '%s' differs from the fresh context's" % tag
    assert res["bad_code"] == 1     # SPP_NOT_POSDEF


def _listed(res):
    return {(i, j) for i, w in enumerate(res["mask"]) for j in range(64) if (w >> j) & 1}


@pytest.mark.parametrize("name", ["chain90", "ba_ring300", "chain73", "loop73", "edges73_aligned"])
def test_repeated_solves_equal_a_fresh_context(name):
    res = _run(name, {}, posv=True)
    _all_equal(res)
    # (the streamed factor works on tiles of the n_red x n_red matrix whatever the block width: all of its tile rows)
    assert res["tile_rows"] == TILE_ROWS[name] and res["streamed"] == [TILE_ROWS[name]] * len(res["streamed"])
    if name in ("chain73", "loop73", "edges73_aligned"):   # only the loop takes a camera order: the branch at the end runs for the others
        assert res["cam_order_used"] == (name == "loop73")
    # the first solve clears the new buffer whole; every later one, the one behind the failed pivot included, by tiles
    assert res["clear"][0] == 0 and set(res["clear"][1:]) == {1}, res["clear"]
    # the tiles that hold anything are the same behind the full clear and behind every clear by tiles
    for t in res["tiles"][1:]:
        assert t == res["tiles"][0]
    n_upper = TILE_ROWS[name] * (TILE_ROWS[name] + 1) // 2
    assert len(res["tiles"][0]) < n_upper, "the case has no empty tile"
    if not res["cam_order_used"]:   # the plan's mask is the natural order's: every tile outside it is exactly zero
        # (edges73_aligned fills its last tile row exactly: behind the mask's rows lies one tile row of padding alone, the
        # identity on its diagonal tile, cleared whole and written by dense_set_padding every time)
        behind = {tuple(t) for t in res["tiles"][0] if t[0] >= res["tile_rows"]}
        assert behind == ({(7, 7)} if name == "edges73_aligned" else set()), behind
        assert {tuple(t) for t in res["tiles"][0]} - behind <= _listed(res)
    if name == "edges73_aligned":
        assert [0, 1] in res["tiles"][0] and [1, 2] in res["tiles"][0], "the corners of the straddling diagonal blocks"


def test_unlisted_tiles_stay_zero_on_the_ring_in_the_natural_order():
    _unlisted_tiles_stay_zero("ba_ring300")


def test_unlisted_tiles_stay_zero_on_the_7_wide_loop_in_the_natural_order():
    """every camera that straddles a tile boundary puts its blocks of S into two tiles per direction: all of them listed"""
    _unlisted_tiles_stay_zero("loop73")


def _unlisted_tiles_stay_zero(name):
    res = _run(name, {"SPP_SCHUR_CAM_ORDER": "0"}, cam_order=False)
    _all_equal(res)
    assert set(res["clear"][1:]) == {1}
    listed = _listed(res)
    assert len(listed) < TILE_ROWS[name] * (TILE_ROWS[name] + 1) // 2
    for t in res["tiles"]:
        assert t, "the S buffer holds nothing"
        assert {tuple(x) for x in t} <= listed, sorted({tuple(x) for x in t} - listed)


@pytest.mark.parametrize("env", [{"SPP_DENSE_TAIL": "0"}, {"SPP_TAIL_MASK": "0"}], ids=["per-step", "unmasked"])
def test_fallback_schedules_force_the_full_clear(env):
    res = _run("chain90", env)
    _all_equal(res)
    assert set(res["clear"]) == {0}, res["clear"]


def test_side_stream_with_the_clear_by_tiles():
    # padding and status reset on the side stream (forced: the shapes are small), beside the clear by tiles
    res = _run("chain90", {"SPP_SCHUR_SIDE": "2"})
    _all_equal(res)
    assert set(res["side"]) == {1} and set(res["clear"][1:]) == {1}
