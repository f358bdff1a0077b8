"""The clear of the solver's own dense S buffer by listed tiles. Invariant: a tile of S outside the filled mask is zero
whenever a factorization starts. The fully masked streamed launch keeps it (a tile without a workgroup is never written),
so the next spp_factor_solve_device clears the listed tiles alone; every other schedule marks the buffer and the next call
clears all of it.

A stale tile can only show where the mask has holes: an open chain of 90 cameras (5 tile rows, tiles (0, 2), (0, 3), (1, 3)
empty) and the 300-camera ring of tests/test_gpu_dense_tilemask.py (15 tile rows). In ONE context values A, values B, then A
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
TILE_ROWS = {"chain90": 5, "ba_ring300": 15}


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


@pytest.mark.parametrize("name", ["chain90", "ba_ring300"])
def test_repeated_solves_equal_a_fresh_context(name):
    res = _run(name, {}, posv=True)
    _all_equal(res)
    assert res["tile_rows"] == TILE_ROWS[name] and res["streamed"] == [TILE_ROWS[name]] * len(res["streamed"])
    # the first solve clears the new buffer whole; every later one, the one behind the failed pivot included, by tiles
    assert res["clear"][0] == 0 and set(res["clear"][1:]) == {1}, res["clear"]
    # the tiles that hold anything are the same behind the full clear and behind every clear by tiles
    for t in res["tiles"][1:]:
        assert t == res["tiles"][0]
    n_upper = TILE_ROWS[name] * (TILE_ROWS[name] + 1) // 2
    assert len(res["tiles"][0]) < n_upper, "the case has no empty tile"
    if not res["cam_order_used"]:   # the plan's mask is the natural order's: every tile outside it is exactly zero
        assert {tuple(t) for t in res["tiles"][0]} <= _listed(res)


def test_unlisted_tiles_stay_zero_on_the_ring_in_the_natural_order():
    res = _run("ba_ring300", {"SPP_SCHUR_CAM_ORDER": "0"}, cam_order=False)
    _all_equal(res)
    assert set(res["clear"][1:]) == {1}
    listed = _listed(res)
    assert len(listed) < 15 * 16 // 2
    for t in res["tiles"]:
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
