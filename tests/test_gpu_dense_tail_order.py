"""GPU: the streamed dense factor with the trailing tile rows seated early (SPP_TAIL_EARLY) against the
same launch numbered row by row. Only the table workgroup -> tile differs; every tile sums its updates in the same order
(steps ascending, row tiles ascending), so factor and solution must be IDENTICAL BITS, and a non-positive pivot must be
reported alike. The switch is read once per process: each value runs in a child process of its own, as the tile-mask
test does. The launch reports the table it built on stderr (SPP_VERBOSE); it must be the one spp_tail_order_host gives
for the device's resident count. Nothing here provokes a timeout."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from slam_plus_plus_amd import api

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB, BS = 128, 6

# (kind, n): 15 to 44 tile rows. "band+wideborder": the border is half the matrix -- its triangle is more than half a
# device of 256 workgroups, the condition refuses it
CASES = [("band", 1920), ("band+border", 3333), ("arrow", 3840), ("band+border", 4000), ("band+border", 5226),
         ("band+wideborder", 5226), ("arrow", 5500), ("band", 5632)]
# (kind, n, row of the failing pivot): inside the rows seated early, in front of them, the very first
BAD = [("band+border", 5226, 4800), ("band+border", 5226, 2000), ("band+border", 4000, 0)]

CHILD = r"""
import hashlib, json, sys
import numpy as np
sys.path.insert(0, %r)
from slam_plus_plus_amd import api

NB, BS = 128, 6

def blocks(kind, nblk):
    I, J = np.triu_indices(nblk)
    w = max(2, nblk // 10)
    if kind == "band":
        keep = J - I <= w
    elif kind == "band+border":
        keep = (J - I <= w) | (J >= nblk - max(3, nblk // 8))
    elif kind == "band+wideborder":
        keep = (J - I <= w) | (J >= nblk // 2)
    elif kind == "arrow":
        keep = (I == J) | (J >= nblk - 4)
    return I[keep], J[keep]

def spd(kind, n, seed):
    nblk = -(-n // BS)
    I, J = blocks(kind, nblk)
    rng = np.random.default_rng(seed)
    P = np.zeros((nblk, nblk), bool)
    P[I, J] = True
    E = np.kron(P, np.ones((BS, BS), bool))[:n, :n]
    A = np.where(E, rng.standard_normal((n, n)), 0.0)
    A = np.triu(A, 1)
    A = A + A.T
    A[np.diag_indices(n)] = np.abs(A).sum(axis=1) + 1.0 + rng.random(n)
    return A, I, J, rng.standard_normal(n)

def posv(ctx, A, b, words):
    n = A.shape[0]
    dA = api.DeviceArray.from_host(ctx, np.asfortranarray(A).reshape(-1, order="F"))
    db = api.DeviceArray.from_host(ctx, b)
    st = ctx._check(ctx.lib.spp_dense_posv_masked(ctx.h, dA.ptr, n, n, db.ptr, words.ctypes.data, words.size))
    streamed = ctx.info("DENSE_STREAMED")
    R = np.triu(dA.download().reshape((n, n), order="F"))
    x = db.download()
    dA.free(); db.free()
    return st, R, x, streamed

cases, bad = json.loads(sys.argv[1]), json.loads(sys.argv[2])
ctx = api.Context(0, 0)
out = []
for kind, n in cases:
    A, I, J, b = spd(kind, n, n)
    words, _ = api.tile_mask_host(n, BS, I, J, True, True)
    words = np.ascontiguousarray(words, dtype=np.uint64)
    st, R, x, streamed = posv(ctx, A, b, words)
    res = float(np.abs(A @ x - b).max() / np.abs(b).max()) if st == 0 else -1.0
    st2, R2, x2, _ = posv(ctx, A, b, words)
    out.append(dict(st=int(st), streamed=int(streamed), res=res, again=bool(st2 == st and np.array_equal(R, R2) and np.array_equal(x, x2)),
                    R=hashlib.sha256(R.tobytes()).hexdigest(), x=hashlib.sha256(x.tobytes()).hexdigest()))
for kind, n, row in bad:
    A, I, J, b = spd(kind, n, n + 1)
    words, _ = api.tile_mask_host(n, BS, I, J, True, True)
    words = np.ascontiguousarray(words, dtype=np.uint64)
    A[row, row] = -1.0
    st, _, _, _ = posv(ctx, A, b, words)
    # ... and the context factors the repaired matrix afterwards
    A[row, row] = np.abs(A[row]).sum() + 1.0
    st2, R, x, streamed = posv(ctx, A, b, words)
    res = float(np.abs(A @ x - b).max() / np.abs(b).max()) if st2 == 0 else -1.0
    out.append(dict(st=int(st), st2=int(st2), streamed=int(streamed), res=res,
                    R=hashlib.sha256(R.tobytes()).hexdigest(), x=hashlib.sha256(x.tobytes()).hexdigest()))
ctx.close()
print("RESULT " + json.dumps(out))
"""

LINE = re.compile(r"\[spp\] streamed tail: (\d+) x (\d+) tiles, (\d+) listed, (\d+) resident; (\d+) tiles of rows (\d+)\.\. seated first")


def _run(early):
    env = {k: v for k, v in os.environ.items() if k not in ("SPP_TAIL_EARLY", "SPP_TAIL_MASK", "SPP_TAIL_ORDER_BETA")}
    env.update({"SPP_TAIL_EARLY": early, "SPP_VERBOSE": "1"})
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT, json.dumps(CASES), json.dumps(BAD)],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, "SPP_TAIL_EARLY=%s: exit %d\n%s%s" % (early, r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    tables = {}   # (tile rows, listed tiles) -> (resident, tiles in front, their first row), as the launch reported them
    for m in LINE.finditer(r.stderr):
        Tr, Tc, listed, resident, ne, rs = (int(v) for v in m.groups())
        tables[(Tr, listed)] = (resident, ne, rs)
    return json.loads(line[7:]), tables


def _words(kind, n):
    nblk = -(-n // BS)
    I, J = np.triu_indices(nblk)
    w = max(2, nblk // 10)
    keep = {"band": J - I <= w, "band+border": (J - I <= w) | (J >= nblk - max(3, nblk // 8)),
            "band+wideborder": (J - I <= w) | (J >= nblk // 2), "arrow": (I == J) | (J >= nblk - 4)}[kind]
    words, _ = api.tile_mask_host(n, BS, I[keep], J[keep], True, True)
    return words


def test_early_and_row_by_row_give_identical_bits_and_report_a_failed_pivot_alike():
    on, tab_on = _run("1")
    off, tab_off = _run("0")
    assert len(on) == len(off) == len(CASES) + len(BAD)
    for q, (kind, n) in enumerate(CASES):
        a, b = on[q], off[q]
        Tr = -(-n // NB)
        assert 15 <= Tr <= 44
        assert a["st"] == 0 and b["st"] == 0 and a["streamed"] == Tr and b["streamed"] == Tr, (kind, n, a, b)
        assert 0 <= a["res"] < 1e-12 and a["again"] and b["again"], (kind, n, a, b)
        assert a["R"] == b["R"], (kind, n, "R differs between SPP_TAIL_EARLY=1 and =0")
        assert a["x"] == b["x"], (kind, n, "x differs between SPP_TAIL_EARLY=1 and =0")
    for q, (kind, n, row) in enumerate(BAD):
        a, b = on[len(CASES) + q], off[len(CASES) + q]
        assert a["st"] == api.SPP_NOT_POSDEF and b["st"] == a["st"], (kind, n, row, a, b)
        assert a["st2"] == 0 and b["st2"] == 0 and 0 <= a["res"] < 1e-12, (kind, n, row, a, b)
        assert a["R"] == b["R"] and a["x"] == b["x"], (kind, n, row)
    # the tables the launches used: with the switch off nothing in front; with it on what the host function says for
    # the device's resident count
    seated = {}
    for kind, n in CASES:
        words = _words(kind, n)
        Tr, listed = len(words), sum(bin(int(w)).count("1") for w in words)
        assert (Tr, listed) in tab_on and (Tr, listed) in tab_off, (kind, n, sorted(tab_on))
        assert tab_off[(Tr, listed)][1] == 0, (kind, n, tab_off[(Tr, listed)])
        resident, ne, rs = tab_on[(Tr, listed)]
        assert resident > 0
        _, info = api.tail_order_host(n, words, True, resident, True)
        assert (ne, rs) == (info["n_early"], info["r_star"]), (kind, n, resident, ne, rs, info)
        seated[(kind, n)] = (resident, ne, rs)
    print(seated)
    resident = seated[("band+border", 5226)][0]
    if resident >= 200:   # (an MI355X holds 256: one workgroup per CU)
        assert seated[("band+border", 5226)][1] > 0, "the bordered case does not seat any tile early"
    # the wide border lags in every row but is more than half of the device: refused, the old table
    _, info = api.tail_order_host(5226, _words("band+wideborder", 5226), True, resident, True)
    assert info["r_star"] == 41 and seated[("band+wideborder", 5226)][1] == 0
    tiles, _ = api.tail_order_host(5226, _words("band+wideborder", 5226), True, resident, True)
    assert tiles == sorted(tiles)
