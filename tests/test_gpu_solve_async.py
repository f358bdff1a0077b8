"""Solve stage with the status off the critical path (SPP_SOLVE_ASYNC, DESIGN "Solve stage: the status leaves the critical
path"): with a dense reduced system spp_factor_solve_device / spp_schur_finish return when the factor's status is known and
leave the triangular solves and the back-substitution running; the chain kernel's timeout word no longer travels on the
stream. The same kernels run with the same arguments in the same order on the ctx stream, so x must have the bits of the
drained order (switch 0), be bit-reproducible, and sit inside the bound of the float64 reference of tests/schur_ref.py.

The switch is read once per process: every value is a child process (tests/solve_async_child.py, which lists the cases).
SPP_INFO_SOLVE_ASYNC tells what each solve did and is asserted too. No test provokes a timed-out chain."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import schur_ref
import test_gpu_cam_order as loop
from solve_async_child import small_system

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "solve_async_child.py")
SMALL = ("edges63", "ba_small", "edges73")
LOOPS = ("loop300", "loop73")   # (name in the child's result; loop300 is loop.system("loop"))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """switch value / options -> (result, solutions), each child started once, on first use"""
    tmp = tmp_path_factory.mktemp("solve_async")
    cache = {}

    def run(switch, **opt):
        key = (switch, tuple(sorted(opt.items())))
        if key not in cache:
            env = {k: v for k, v in os.environ.items() if k != "SPP_SOLVE_ASYNC"}
            if switch is not None:
                env["SPP_SOLVE_ASYNC"] = str(switch)
            out = str(tmp / ("x_%d.npz" % len(cache)))
            r = subprocess.run([sys.executable, CHILD, out, json.dumps(opt)], env=env, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, "%s: exit %d\n%s%s" % (key, r.returncode, r.stdout[-3000:], r.stderr[-3000:])
            res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            print(key, {k: v.get("asy") for k, v in res.items() if isinstance(v, dict)})
            cache[key] = (res, dict(np.load(out)))
        return cache[key]
    return run


@pytest.fixture(scope="module")
def references():
    """name -> (reference, lam, eta), computed once"""
    refs = {}
    for name in SMALL:
        lam, eta = small_system(name)
        refs[name] = (schur_ref.schur_ref(lam, eta, schur_ref.guided_elim(lam)), lam, eta)
    return refs


def _took(res, want):
    for name in SMALL + LOOPS:
        assert res[name]["asy"] == [want, want], (name, res[name]["asy"])
    assert res["six in a row"]["asy"] == [want] * 6
    assert res["two shards"]["asy"] == [want, want]
    for tag, b in res["bad pivots"].items():
        assert b["asy"] == want, (tag, b)


def _same_bits(a, b, what):
    for name in SMALL + LOOPS + ("two shards",):
        assert a[name]["x"] == b[name]["x"], (what, name, "x differs")


def test_the_shapes_reach_the_code(runs):
    res, _ = runs(1)
    assert res["loop300"]["tile_rows"] == 15 and res["loop300"]["streamed"] > 0, "the streamed factor did not run on the loop"
    assert res["loop300"]["order"] != list(range(loop.NC)), "the loop's camera order (arcs, separators) was not taken"
    assert res["ba_small"]["tile_rows"] == 2, res["ba_small"]   # the smoke problem: the shortest chain there is
    # (edges63 is 320 cameras, 15 tile rows like the loop, with the pair-count spread of tests/schur_fixtures.py)
    assert res["edges63"]["tile_rows"] == 15, res["edges63"]
    # 7-wide cameras: 17.5 tiles (the rhs column inside the last tile), and a loop of 19 tile rows in its camera order
    assert res["edges73"]["tile_rows"] == 18 and res["edges73"]["streamed"] > 0, res["edges73"]
    assert res["loop73"]["tile_rows"] == 19 and res["loop73"]["streamed"] > 0, "the streamed factor did not run on the 7-wide loop"
    assert res["loop73"]["order"] != list(range(330)) and sorted(res["loop73"]["order"]) == list(range(330))


def test_early_status_gives_the_bits_of_the_drained_order(runs):
    serial, early, default = runs(0)[0], runs(1)[0], runs(None)[0]
    _took(serial, 0)
    _took(early, 1)
    _took(default, 1)
    _same_bits(early, serial, "SPP_SOLVE_ASYNC=1 against =0")
    _same_bits(default, serial, "the default against SPP_SOLVE_ASYNC=0")
    for res in (serial, early):
        for name in SMALL + LOOPS:
            assert res[name]["repro"], (name, "x not bit-reproducible")


@pytest.mark.parametrize("switch", [0, 1])
def test_solutions_are_inside_the_bound_of_the_reference(runs, references, switch):
    res, xs = runs(switch)
    for name in SMALL:
        R, lam, eta = references[name]
        assert res[name]["order"] == list(range(len(res[name]["order"]))), "%s: natural camera order expected" % name
        print(name, "landmark / pose part, error / bound:", schur_ref.check_solution(R, lam, eta, xs[name]))
    lam, eta = loop.system("loop")
    P = loop._ref_in_order(lam, eta, np.asarray(res["loop300"]["order"]))
    print("loop300 landmark / pose part, error / bound:", schur_ref.check_solution(P, lam, eta, xs["loop300"]))
    lam, eta = loop.system("loop73")
    P = loop._ref_in_order(lam, eta, np.asarray(res["loop73"]["order"]), "loop73")
    print("loop73 landmark / pose part, error / bound:", schur_ref.check_solution(P, lam, eta, xs["loop73"]))


@pytest.mark.parametrize("switch", [0, 1])
def test_six_solves_enqueued_back_to_back_equal_the_solves_done_alone(runs, switch):
    six = runs(switch)[0]["six in a row"]
    assert six["codes"] == [0] * 6
    assert six["equal"] == [True] * 6, six["equal"]


@pytest.mark.parametrize("where", ["first tile", "arc B", "separator"])
def test_a_non_positive_pivot_is_reported_and_the_next_solve_is_good(runs, where):
    """(the C ABI reports SPP_NOT_POSDEF, not the index of the pivot: the return codes are what can be compared)"""
    serial, early = runs(0)[0]["bad pivots"][where], runs(1)[0]["bad pivots"][where]
    assert serial["code"] == 1 and early["code"] == serial["code"]
    for b in (serial, early):
        assert b["code_good"] == 0 and b["good_equal"], b   # the status reset is intact: the bits of the first good solve


def test_profiling_keeps_the_drained_order_and_the_bits(runs):
    prof = runs(1, profile=True)[0]
    _took(prof, 0)
    _same_bits(prof, runs(0)[0], "profiling on against SPP_SOLVE_ASYNC=0")
    assert prof["six in a row"]["equal"] == [True] * 6
