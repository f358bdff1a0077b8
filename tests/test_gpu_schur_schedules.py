"""Every switch of the Schur stage, against the longdouble reference and against each other's bits.

The S accumulation and the back-substitution read their switches once per process (hence one child process per variant,
run one after the other): SPP_SACC_CHUNK (items per wave; 0 = one persistent set of workgroups, > 1 = the prefetch of the
next item), SPP_SACC_TILE / SPP_SACC_TILE_COLS / SPP_SACC_XCD (the order of the work items and their deal to the XCDs),
SPP_SACC_FACTORED / SPP_SACC_ULM (the operands: one packed block per observation, or W and U, landmark- or camera-major),
SPP_BACKSUBST_FUSED (one launch, or the products U^T dx through memory).

Each child forms S | rhs and solves the edge fixtures of tests/schur_fixtures.py (6-, 3- and one-width cases) or of
tests/schur_fixtures_73.py (7-wide cameras) twice (bit-reproducible), checks both
against the reference itself and prints sha256 of S | rhs and of x. The parent demands the default's bits wherever the
variant may change only the item order, the item-to-wave assignment or where an operand is stored: the sum of an item is
fixed by its pair list."""
import json
import os
import pickle
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import schur_fixtures_73 as fx73
import schur_ref
from slam_plus_plus_amd import api

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
CASES = [("edges63", api.MODE_SCHUR), ("edges63_long", api.MODE_SCHUR), ("edges32", api.MODE_SCHUR),
         ("mis66", api.MODE_SCHUR_MIS)]
# 7-wide cameras, 3-wide points (tests/schur_fixtures_73.py): the instantiations <7, 3> of every kernel the switches select --
# the unfactored operands and the unfused back-substitution run nowhere else -- and the item pipeline at 21 doubles per
# block. A child of their own per variant: each child keeps its time limit.
CASES_73 = [("edges73", api.MODE_SCHUR), ("edges73_aligned", api.MODE_SCHUR)]

CHILD = r"""
import hashlib, json, pickle, sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
from slam_plus_plus_amd import api
import schur_fixtures_73 as fx73
import schur_ref

refs = pickle.load(open(sys.argv[1], "rb"))
out = {}
for name, mode in json.loads(sys.argv[2]):
    lam, eta = fx73.make_any(name)
    R = refs[name]
    ctx = api.Context(0, 0)
    ctx.analyze(lam, mode)
    elim = np.sort(ctx.ordering(lam.nb)[lam.nb - ctx.info("N_LANDMARKS"):])
    assert np.array_equal(elim, R.elim), name
    dv = api.DeviceArray.from_host(ctx, lam.vals)
    dr = api.DeviceArray(ctx, lam.n)
    dS = api.DeviceArray(ctx, ctx.schur_buffer_size())
    bufs, xs = [], []
    for rep in range(2):
        dr.upload(eta)
        ctx.schur_form(dv.ptr, dr.ptr, dS.ptr)
        ctx.synchronize()
        bufs.append(dS.download())
        assert ctx.factor_solve_device(dv.ptr, dr.ptr) == 0
        xs.append(dr.download())
    assert np.array_equal(bufs[0], bufs[1]), "%%s: S | rhs not bit-reproducible" %% name
    assert np.array_equal(xs[0], xs[1]), "%%s: x not bit-reproducible" %% name
    rs = schur_ref.check_schur_buffer(R, bufs[0], mode != api.MODE_SCHUR, ctx.info("S_LD"))
    rl, rc = schur_ref.check_solution(R, lam, eta, xs[0])
    out[name] = dict(S=hashlib.sha256(bufs[0].tobytes()).hexdigest(), x=hashlib.sha256(xs[0].tobytes()).hexdigest(),
                     ratio_S=rs, ratio_xl=rl, ratio_xc=rc)
    for d in (dv, dr, dS):
        d.free()
    ctx.close()
print("RESULT " + json.dumps(out))
"""

VARIANTS = [  # (tag, environment, same S | rhs as the default, same x as the default)
    ("chunk0", {"SPP_SACC_CHUNK": "0"}, True, True),
    ("chunk2", {"SPP_SACC_CHUNK": "2"}, True, True),
    ("chunk5", {"SPP_SACC_CHUNK": "5"}, True, True),
    ("tile1", {"SPP_SACC_TILE": "1"}, True, True),
    ("tile3", {"SPP_SACC_TILE": "3"}, True, True),
    ("cols0", {"SPP_SACC_TILE_COLS": "0"}, True, True),
    ("xcd0", {"SPP_SACC_XCD": "0"}, True, True),
    ("bsfused0", {"SPP_BACKSUBST_FUSED": "0"}, True, True),
    ("fact0", {"SPP_SACC_FACTORED": "0"}, False, False),
    ("fact0ulm0", {"SPP_SACC_FACTORED": "0", "SPP_SACC_ULM": "0"}, False, False),
]
SWITCHES = ["SPP_SACC_CHUNK", "SPP_SACC_TILE", "SPP_SACC_TILE_COLS", "SPP_SACC_XCD", "SPP_BACKSUBST_FUSED",
            "SPP_SACC_FACTORED", "SPP_SACC_ULM"]


def _run(env_extra, refs_path):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(env_extra)
    out = {}
    for cases in (CASES, CASES_73):   # one child after the other; a non-zero exit ends the test
        r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, TESTS), refs_path, json.dumps(cases)], env=env,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, "%s: exit %d\n%s%s" % (env_extra, r.returncode, r.stdout[-3000:], r.stderr[-3000:])
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        out.update(json.loads(line[7:]))
    return out


def _references(ctx_modes):
    """the reference of every case, computed once here and kept compact (the layout of its mode, the bounds, the pose
    solution: no dense S or M); the children read it from a file"""
    refs = {}
    c = api.Context(0)
    for name, mode in ctx_modes:
        lam, eta = fx73.make_any(name)
        c.analyze(lam, mode)
        elim = np.sort(c.ordering(lam.nb)[lam.nb - c.info("N_LANDMARKS"):])
        R = schur_ref.schur_ref(lam, eta, elim).compact(dense=mode == api.MODE_SCHUR, sparse=mode != api.MODE_SCHUR)
        R.elim = elim
        refs[name] = R
    c.close()
    return refs


def test_every_schur_switch():
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "refs.pkl")
        with open(path, "wb") as f:
            pickle.dump(_references(CASES + CASES_73), f)
        base = _run({}, path)
        print("default", {k: "S %.3f xl %.3f xc %.3f" % (v["ratio_S"], v["ratio_xl"], v["ratio_xc"]) for k, v in base.items()})
        got = {}
        for tag, env, same_s, same_x in VARIANTS:   # one child at a time; the first failure ends the test
            got[tag] = g = _run(env, path)
            print(tag, {k: "S %.3f xl %.3f xc %.3f" % (v["ratio_S"], v["ratio_xl"], v["ratio_xc"]) for k, v in g.items()})
            for name, _ in CASES + CASES_73:
                if same_s:
                    assert g[name]["S"] == base[name]["S"], (tag, name, "S | rhs differs from the default")
                if same_x:
                    assert g[name]["x"] == base[name]["x"], (tag, name, "x differs from the default")
        # SPP_SACC_ULM moves only where U is stored: the same operations in the same order
        for name, _ in CASES + CASES_73:
            assert got["fact0"][name]["S"] == got["fact0ulm0"][name]["S"], name
            assert got["fact0"][name]["x"] == got["fact0ulm0"][name]["x"], name
