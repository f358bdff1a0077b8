"""Every schedule of the dense factor and every form of its backward substitution, on one list of sizes.

dense_factor_steps picks, by size and by switches the library reads once per process (hence one child process per
variant, run one after the other): the streamed launch (spp_dense_tail.h: a whole factorization of up to 44 tile rows, or
the tail of a bigger one from the step where at most 44 remain), the two-stream per-step schedule with device-flag or
event hand-offs, the fused chain kernel, the lookahead schedule, and three forms of the 128 x 128 tiles of the trailing
update; dense_potrs_upper one of four substitution forms.

Each child factors and solves 129 .. 7000 (5632 = 44 tile rows is the last size streamed whole, 5633 the first that hands
over), checks the result itself, repeats it for bit-reproducibility, and reports per size the tile rows the streamed
launch took (SPP_INFO_DENSE_STREAMED) and sha256 of R and x. The parent checks the path taken against a table -- a changed
threshold cannot reroute these tests silently -- and the bits against the default wherever the variant may change only
hand-offs, workgroup order or the solve."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [129, 640, 1000, 2688, 3201, 4224, 5632, 5633, 7000]

CHILD = r"""
import hashlib, json, sys
import numpy as np
sys.path.insert(0, %r)
from slam_plus_plus_amd import api

def spd(n):   # rank 64 + diagonal: O(n^2 r) to build
    rng = np.random.default_rng(n)
    V = rng.standard_normal((n, 64))
    A = V @ V.T / 64
    A[np.diag_indices(n)] += 1.0 + rng.random(n)
    return A, rng.standard_normal(n)

ctx = api.Context(0, 0)
out = {}
for n in json.loads(sys.argv[1]):
    A, b = spd(n)
    runs = []
    for rep in range(2):
        dA = api.DeviceArray.from_host(ctx, A.reshape(-1))   # symmetric: row-major == column-major
        db = api.DeviceArray.from_host(ctx, b)
        assert ctx._check(ctx.lib.spp_dense_posv(ctx.h, dA.ptr, n, n, db.ptr)) == 0
        streamed = ctx.info("DENSE_STREAMED")
        R = np.triu(dA.download().reshape((n, n), order="F"))
        x = db.download()
        dA.free(); db.free()
        runs.append((R, x, streamed))
    (R, x, streamed), (R2, x2, streamed2) = runs
    assert np.array_equal(R, R2) and np.array_equal(x, x2) and streamed == streamed2, "n %%d: not bit-reproducible" %% n
    amax = np.abs(A).max()
    if n <= 1000:
        ferr = np.abs(R.T @ R - A).max() / amax
    else:   # four random probes: |(R^T R - A) v| <= ferr |A|_max |v|_1
        P = np.random.default_rng(1).standard_normal((n, 4))
        ferr = (np.abs(R.T @ (R @ P) - A @ P).max(axis=0) / np.abs(P).sum(axis=0)).max() / amax
    res = np.abs(A @ x - b).max() / np.abs(b).max()
    assert ferr < 1e-13, (n, ferr)
    assert res < 1e-12, (n, res)
    out[n] = dict(streamed=streamed, ferr=ferr, res=res, R=hashlib.sha256(R.tobytes()).hexdigest(),
                  x=hashlib.sha256(x.tobytes()).hexdigest())
print("RESULT " + json.dumps(out))
"""

# tile rows the streamed launch takes, per size (nsteps = 2, 5, 8, 21, 26, 33, 44, 45, 55)
DEFAULT_PATH = [2, 5, 8, 21, 26, 33, 44, 44, 44]
VARIANTS = [  # (tag, environment, expected DENSE_STREAMED, same R as the default, same x as the default)
    ("sched0", {"SPP_DENSE_SCHED": "0"}, DEFAULT_PATH, "all", True),
    ("beta", {"SPP_TAIL_ORDER_BETA": "0.5"}, DEFAULT_PATH, "all", True),
    ("tail0", {"SPP_DENSE_TAIL": "0"}, [0] * 9, "none", False),
    ("rows8", {"SPP_TAIL_ROWS": "8"}, [2, 5, 8, 8, 8, 8, 8, 8, 8], "none", False),
    ("rows2", {"SPP_TAIL_ROWS": "2"}, [2] * 9, "none", False),
    ("fused0", {"SPP_FUSED": "0"}, DEFAULT_PATH, "whole", False),
    ("tile1", {"SPP_TILE_444": "1"}, DEFAULT_PATH, "whole", False),
    ("tile2", {"SPP_TILE_444": "2"}, DEFAULT_PATH, "whole", False),
    ("la", {"SPP_DENSE_LA": "1"}, [2, 5, 0, 0, 0, 0, 0, 0, 0], "none", False),   # lookahead from 6 steps on
    ("chain0", {"SPP_TRSV_CHAIN": "0"}, DEFAULT_PATH, "all", False),
    ("chain1", {"SPP_TRSV_CHAIN": "1"}, DEFAULT_PATH, "all", False),
    ("mform0", {"SPP_TRSV_MFORM": "0"}, DEFAULT_PATH, "all", False),
]
SWITCHES = ["SPP_DENSE_SCHED", "SPP_TAIL_ORDER_BETA", "SPP_DENSE_TAIL", "SPP_TAIL_ROWS", "SPP_FUSED", "SPP_TILE_444",
            "SPP_DENSE_LA", "SPP_TRSV_CHAIN", "SPP_TRSV_MFORM", "SPP_TAIL_TIMEOUT_TICKS", "SPP_CHAIN_TIMEOUT_TICKS"]


def _child(code, args, env_extra, timeout):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(env_extra)
    return subprocess.run([sys.executable, "-c", code] + args, env=env, capture_output=True, text=True, timeout=timeout)


def _run(env_extra):
    r = _child(CHILD % ROOT, [json.dumps(SIZES)], env_extra, 240)
    assert r.returncode == 0, "%s: exit %d\n%s%s" % (env_extra, r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return {int(k): v for k, v in json.loads(line[7:]).items()}


def test_every_dense_schedule_and_substitution_form():
    base = _run({})
    seen = {"default": [base[n]["streamed"] for n in SIZES]}
    assert seen["default"] == DEFAULT_PATH, seen
    for tag, env, path, same_r, same_x in VARIANTS:   # one child at a time; the first failure ends the test
        got = _run(env)
        seen[tag] = [got[n]["streamed"] for n in SIZES]
        print(tag, seen[tag], "max factor err %.1e" % max(got[n]["ferr"] for n in SIZES))
        assert seen[tag] == path, (tag, seen[tag], path)
        for n, streamed in zip(SIZES, path):
            whole = streamed * 128 >= n        # the whole factorization was the streamed launch
            if same_r == "all" or (same_r == "whole" and whole):
                assert got[n]["R"] == base[n]["R"], (tag, n, "R differs from the default")
            if same_x:
                assert got[n]["x"] == base[n]["x"], (tag, n, "x differs from the default")


TIMEOUT_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, %r)
from slam_plus_plus_amd import api
n = 3000
rng = np.random.default_rng(3)
V = rng.standard_normal((n, 64))
A = V @ V.T / 64
A[np.diag_indices(n)] += 1.0 + rng.random(n)
ctx = api.Context(0, 0)
dA = api.DeviceArray.from_host(ctx, A.reshape(-1))
st = ctx.lib.spp_dense_potrf_upper(ctx.h, dA.ptr, n, n)
msg = ctx.last_error()
assert st == -3, (st, msg)   # SPP_E_HIP
assert "streamed launch" in msg, msg
print("first call:", msg)
for rep in range(2):
    dA.upload(A.reshape(-1))
    assert ctx._check(ctx.lib.spp_dense_potrf_upper(ctx.h, dA.ptr, n, n)) == 0
    assert ctx.info("DENSE_STREAMED") == 0
    R = np.triu(dA.download().reshape((n, n), order="F"))
    P = np.random.default_rng(rep).standard_normal((n, 4))
    err = (np.abs(R.T @ (R @ P) - A @ P).max(axis=0) / np.abs(P).sum(axis=0)).max() / np.abs(A).max()
    assert err < 1e-13, err
    Rref = np.linalg.cholesky(A).T
    assert np.abs(R - Rref).max() / np.abs(Rref).max() < 1e-11
print("TIMEOUT OK")
"""


def test_timed_out_streamed_launch_falls_back_to_the_per_step_schedule():
    """SPP_TAIL_TIMEOUT_TICKS=1 makes the streamed launch's first wait for a tile give up (a bounded wait the kernel
    handles, as the sparse DAG's SPP_DAG_TIMEOUT_TICKS): the call fails with an error that names the streamed launch, and
    the following factorizations on the context take the per-step schedule and are right"""
    r = _child(TIMEOUT_CHILD % ROOT, [], {"SPP_TAIL_TIMEOUT_TICKS": "1"}, 180)
    assert r.returncode == 0 and "TIMEOUT OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


CHAIN_TIMEOUT_CHILD = r"""
import hashlib, sys
import numpy as np
sys.path.insert(0, %r)
from slam_plus_plus_amd import api
n = 640   # five block rows: two is the smallest size at which a workgroup of the one-hop-per-workgroup chain waits at all,
          # three the smallest for a helper of the one-workgroup chain; five leaves several waiters
rng = np.random.default_rng(5)
V = rng.standard_normal((n, 64))
A = V @ V.T / 64
A[np.diag_indices(n)] += 1.0 + rng.random(n)
b = rng.standard_normal(n)
ctx = api.Context(0, 0)
dA = api.DeviceArray.from_host(ctx, A.reshape(-1))
db = api.DeviceArray.from_host(ctx, b)
if sys.argv[1] == "timeout":
    st = ctx.lib.spp_dense_posv(ctx.h, dA.ptr, n, n, db.ptr)
    msg = ctx.last_error()
    assert st == -3, (st, msg)   # SPP_E_HIP
    assert "backward substitution" in msg and "launch per block row" in msg, msg
    print("first call:", msg)
for rep in range(2):
    dA.upload(A.reshape(-1))
    db.upload(b)
    assert ctx._check(ctx.lib.spp_dense_posv(ctx.h, dA.ptr, n, n, db.ptr)) == 0
    x = db.download()
    res = np.abs(A @ x - b).max() / np.abs(b).max()
    print("residual %%.3e" %% res)
    assert res < 1e-12, res
    print("X " + hashlib.sha256(x.tobytes()).hexdigest())
print("CHAIN TIMEOUT OK")
"""


def test_timed_out_chain_falls_back_to_a_launch_per_block_row():
    """SPP_CHAIN_TIMEOUT_TICKS=1 makes the first wait inside a backward-substitution chain kernel that is not satisfied at
    once give up (a bounded wait the kernel handles, spp_wait.h): the call fails with an error that names the backward
    substitution and the fallback, and the following solves on the context launch per block row -- right, and bit for bit
    what SPP_TRSV_CHAIN=0 gives"""
    def xs(env, mode):
        r = _child(CHAIN_TIMEOUT_CHILD % ROOT, [mode], env, 120)
        assert r.returncode == 0 and "CHAIN TIMEOUT OK" in r.stdout, "%s\n%s%s" % (env, r.stdout[-3000:], r.stderr[-3000:])
        print(env, r.stdout)
        return [ln for ln in r.stdout.splitlines() if ln.startswith("X ")]
    ref = xs({"SPP_TRSV_CHAIN": "0"}, "plain")
    assert len(ref) == 2 and ref[0] == ref[1]
    for env in ({}, {"SPP_TRSV_MFORM": "0"}, {"SPP_TRSV_CHAIN": "1"}):   # one child at a time
        assert xs(dict(env, SPP_CHAIN_TIMEOUT_TICKS="1"), "timeout") == ref, env
