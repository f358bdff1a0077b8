"""The side stream of the Schur stage (SPP_SCHUR_SIDE): the reduced right-hand side -- and in the one-call path the padding
of S and the status reset -- run beside the S accumulation, ordered against the ctx stream by two events. The same kernels
run with the same arguments, so S | rhs and x must have the bits of the serial order.

The switch is read once per process: every variant is a child process (tests/schur_side_child.py), which forms and solves
each edge fixture of tests/schur_fixtures.py and edges73 (7-wide cameras) twice in one context (bit-reproducible), checks both against the longdouble
reference of tests/schur_ref.py, drives two landmark shards through the split API (form, pack without a synchronization
in between, sum, unpack, finish) and prints sha256 of S | rhs and of x. The fixtures are far below SCHUR_SIDE_MIN_OBS
observations, so the default (1) keeps the serial order on them and SPP_SCHUR_SIDE=2 forces the fork; the children report
which order ran (SPP_INFO_SCHUR_SIDE) and the parent checks that too."""
import json
import os
import pickle
import subprocess
import sys

import pytest

import schur_side_child as child
from test_gpu_schur_schedules import _references

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "schur_side_child.py")
SHARDS = [n + "/2 shards" for n in child.SHARD_CASES]
NAMES = [n for n, _ in child.SIDE_CASES] + SHARDS


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """variant -> result, each child started once, on first use"""
    path = str(tmp_path_factory.mktemp("schur_side") / "refs.pkl")
    with open(path, "wb") as f:
        pickle.dump(_references(child.SIDE_CASES), f)
    cache = {}

    def run(side, **opt):
        key = (side, tuple(sorted(opt.items())))
        if key not in cache:
            env = {k: v for k, v in os.environ.items() if k != "SPP_SCHUR_SIDE"}
            if side is not None:
                env["SPP_SCHUR_SIDE"] = str(side)
            r = subprocess.run([sys.executable, CHILD, "side", path, json.dumps(opt)], env=env, capture_output=True, text=True,
                               timeout=180)
            assert r.returncode == 0, "%s: exit %d\n%s%s" % (key, r.returncode, r.stdout[-3000:], r.stderr[-3000:])
            cache[key] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            print(key, {k: v["side"] for k, v in cache[key].items()})
            print(key, "largest error / bound", {k: "S %.3f xl %.3f xc %.3f" % (v["ratio_S"], v["ratio_xl"], v["ratio_xc"])
                                                 for k, v in cache[key].items() if "ratio_S" in v})
        return cache[key]
    return run


def _same_bits(a, b, what):
    for name in NAMES:
        assert a[name]["S"] == b[name]["S"], (what, name, "S | rhs differs")
        assert a[name]["x"] == b[name]["x"], (what, name, "x differs")


def _took(res, side):
    for name in NAMES:
        assert set(res[name]["side"]) == {side}, (name, res[name]["side"])


def test_side_stream_gives_the_bits_of_the_serial_order(runs):
    serial, forced, default = runs(0), runs(2), runs(None)
    _took(serial, 0)
    _took(forced, 1)
    _took(default, 0)    # below SCHUR_SIDE_MIN_OBS observations the default is the serial order
    _same_bits(forced, serial, "SPP_SCHUR_SIDE=2 against =0")
    _same_bits(default, serial, "the default against SPP_SCHUR_SIDE=0")
    _same_bits(runs(1), serial, "SPP_SCHUR_SIDE=1 against =0")


def test_profiling_keeps_the_serial_order_and_the_bits(runs):
    prof = runs(2, profile=True)
    _took(prof, 0)
    _same_bits(prof, runs(0), "profiling on against SPP_SCHUR_SIDE=0")
    _same_bits(prof, runs(2), "profiling on against off")


def test_adopted_stream_gives_the_same_bits(runs):
    adopted = runs(2, adopt=True)
    _took(adopted, 1)
    _same_bits(adopted, runs(0), "a torch stream adopted with set_stream, SPP_SCHUR_SIDE=2 against =0 on the ctx's own stream")
    _same_bits(runs(0, adopt=True), runs(0), "a torch stream adopted with set_stream, serial order")


def test_split_api_gives_the_bits_of_the_serial_order(runs):
    forced, serial = runs(2), runs(0)
    assert SHARDS == ["edges63/2 shards", "edges73/2 shards"]
    for key in SHARDS:
        assert forced[key]["side"] == [1, 1] and serial[key]["side"] == [0, 0]
        assert forced[key]["S"] == serial[key]["S"]
        assert forced[key]["x"] == serial[key]["x"]
