"""SPP_LM_STREAM: the streamed landmark-side Schur kernels against the one-lane-per-block kernels, bit for bit.

The switch changes only how bytes travel (U fetched cooperatively in 16-byte pieces through a per-wave LDS image, xw in
observation order and gathered by rhs_kernel, the fused back-substitution working through several groups with the next
fetch in flight): per observation, per landmark and per camera the operations and their order stay. So S | rhs and the
solution x must have the same sha256 with the switch at 1 (the default), at 2 (xw camera-major) and at 0, each
bit-reproducible over two runs,
and each inside the bound of tests/schur_ref.py that tests/test_gpu_schur_stage.py uses for the same quantities.

The problems are built with the block builder of tests/schur_fixtures.py; their shapes sit on the edges of the new loops:
  obsN      N = 1, 63, 64, 65, 255, 256, 257, 513 (= 4 * 64 * 2 + 1) observations in all: the last wave and the last
            workgroup of obs_fact_stream_kernel partly empty, the last back-substitution group a single observation
  tracks    camera 0 observes 70 landmarks of its own (the lane-strided rhs sum wraps; camera 1 observes exactly one
            of them), then landmarks with 1, 2, 64, 65 and 256 observers in this order: the 256-observer track is the
            LAST landmark and cannot join the 202 observations before it, so the plan has two back-substitution groups
            and the boundary falls on the last landmark (BS_GROUPS == 2 is asserted)
  tracks257 the same plus a 257-observer track: the whole plan takes backsubst_obs_kernel + backsubst_lm_kernel
            (BS_GROUPS == 0)
  groups9   2100 two-observer landmarks: 17 back-substitution groups of 128 landmarks
  groups1023, groups1025   the same with 1023 and 1025 groups: from 1024 groups on a workgroup of backsubst_stream_kernel
            works through 4 consecutive groups with the next fetch in flight (1025 = 4 * 256 + 1: the last workgroup
            has one group), below that through one
  obs65w32, tracks32   3-wide poses and 2-wide landmarks: widths the streamed kernels are not built for (generic path;
            LM_STREAM reports 0 whatever the switch)
Every child also reports which kernels its schur_form launched (info LM_STREAM): the switch's value for 6 x 3, so a
switch that were ignored would fail the test.
The switch is read once per process: one child process per value, each running every case (and the two-shard case:
set_shard, pack, host sum, unpack, finish)."""
import json
import os
import pickle
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import schur_fixtures as fx
import schur_ref
from slam_plus_plus_amd import api

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
OBS_COUNTS = [1, 63, 64, 65, 255, 256, 257, 4 * 64 * 2 + 1]
TRACKS = [1, 2, 64, 65, 256]
CASES = ["obs%d" % n for n in OBS_COUNTS] + ["tracks", "tracks257", "groups9", "groups1023", "groups1025", "obs65w32", "tracks32"]
BS_GROUPS = {"tracks": 2, "tracks257": 0, "groups9": 17, "groups1023": 1023, "groups1025": 1025}   # what the plan must have built
SHARD_CASE = "tracks"


def _obs_count(n, nc=6):
    """n observations: two-observer landmarks of neighbouring cameras, and a single-observer one when n is odd"""
    obs = []
    for lm in range(n // 2):
        obs += [(lm % nc, lm), ((lm + 1) % nc, lm)]
    if n % 2:
        obs.append(((n // 2) % nc, n // 2))
    return nc, (n + 1) // 2, obs


def _tracks(lengths, nc=264):
    obs = []
    lm = 0
    for q in range(70):                          # camera 0: more than 64 observations
        obs.append((0, lm))
        lm += 1
    obs.append((1, lm - 1))                      # camera 1: exactly one
    for k in lengths:
        obs += [(2 + q, lm) for q in range(k)]   # cameras 2 .. : cameras 0 and 1 stay out of the tracks
        lm += 1
    return nc, lm, obs


def make_case(name):
    """(lam, eta) of a case; module level so that the child processes build the same problems"""
    dp, dl = (3, 2) if name.endswith("32") else (6, 3)
    if name.startswith("obs"):
        nc, nl, obs = _obs_count(int(name[3:].split("w")[0]))
    elif name.startswith("tracks"):
        nc, nl, obs = _tracks(TRACKS + ([257] if name == "tracks257" else []))
    elif name == "groups9":
        nc, nl, obs = _obs_count(4200, nc=20)
    elif name.startswith("groups"):
        nc, nl, obs = _obs_count(256 * int(name[6:]), nc=20)
    else:
        raise KeyError(name)
    a_edges = [(i, i + 1) for i in range(nc - 1)]   # every camera tied to its neighbour, whatever it observes
    return fx._guided(nc, nl, dp, dl, obs, a_edges, seed=len(obs) + dp)


CHILD = r"""
import hashlib, json, pickle, sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
from slam_plus_plus_amd import api
import schur_ref
import test_gpu_lm_stream as T

refs = pickle.load(open(sys.argv[1], "rb"))
sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
out = {}
for name in T.CASES:
    lam, eta = T.make_case(name)
    R = refs[name]
    ctx = api.Context(0, 0)
    ctx.analyze(lam, api.MODE_SCHUR)
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
    rs = schur_ref.check_schur_buffer(R, bufs[0], False, ctx.info("S_LD"))
    rl, rc = schur_ref.check_solution(R, lam, eta, xs[0])
    out[name] = dict(S=sha(bufs[0]), x=sha(xs[0]), ratio_S=rs, ratio_xl=rl, ratio_xc=rc, lm_stream=ctx.info("LM_STREAM"),
                     bs_groups=ctx.info("BS_GROUPS"))
    for d in (dv, dr, dS):
        d.free()
    ctx.close()

# two shards on one device: partial S | rhs, pack, host sum (the all-reduce), unpack, finish
lam, eta = T.make_case(T.SHARD_CASE)
ctxs, bufs, packed = [], [], []
for r in range(2):
    c = api.Context(0)
    c.set_shard(r, 2)
    c.analyze(lam, api.MODE_SCHUR)
    dv = api.DeviceArray.from_host(c, lam.vals)
    dr = api.DeviceArray.from_host(c, eta)
    dS = api.DeviceArray(c, c.schur_buffer_size())
    c.schur_form(dv.ptr, dr.ptr, dS.ptr)
    dP = api.DeviceArray(c, c.schur_packed_size())
    c.schur_pack(dS.ptr, dP.ptr)
    c.synchronize()
    ctxs.append(c)
    bufs.append((dv, dr, dS))
    packed.append(dP)
psum = sum(p.download() for p in packed)
shard = dict(packed=sha(psum), x=[])
for c, (dv, dr, dS), dP in zip(ctxs, bufs, packed):
    dP.upload(psum)
    c.schur_unpack(dP.ptr, dS.ptr)
    assert c.schur_finish(dv.ptr, dS.ptr, dr.ptr) == 0
    c.synchronize()
    shard["x"].append(sha(dr.download()))
out["__shards__"] = shard
print("RESULT " + json.dumps(out))
"""


def _run(value, refs_path):
    env = dict(os.environ)
    env.pop("SPP_LM_STREAM", None)
    if value is not None:
        env["SPP_LM_STREAM"] = value
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, TESTS), refs_path], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, "SPP_LM_STREAM=%s: exit %d\n%s%s" % (value, r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def _references():
    refs = {}
    c = api.Context(0)
    for name in CASES:
        lam, eta = make_case(name)
        c.analyze(lam, api.MODE_SCHUR)
        elim = np.sort(c.ordering(lam.nb)[lam.nb - c.info("N_LANDMARKS"):])
        assert elim.size == int((lam.dim == lam.dim.min()).sum()), name   # every landmark is eliminated
        R = schur_ref.schur_ref(lam, eta, elim).compact(dense=True, sparse=False)
        R.elim = elim
        refs[name] = R
    c.close()
    return refs


def test_cases_have_the_shapes_they_are_named_for():
    """host only in effect (no kernel runs): the observation counts and track lengths the docstring promises"""
    for n in OBS_COUNTS:
        nc, nl, obs = _obs_count(n)
        assert len(obs) == n and len(set(obs)) == n and max(l for _, l in obs) == nl - 1
    nc, nl, obs = _tracks(TRACKS + [257])
    per_lm = np.bincount([l for _, l in obs], minlength=nl)
    assert list(per_lm[-6:]) == TRACKS + [257] and per_lm[:-6].sum() + sum(TRACKS[:4]) <= 256 < per_lm[:-6].sum() + sum(TRACKS)
    per_cam = np.bincount([c for c, _ in obs], minlength=nc)
    assert per_cam[0] == 70 and per_cam[1] == 1 and max(c for c, _ in obs) < nc


def test_streamed_landmark_kernels_keep_every_bit():
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "refs.pkl")
        with open(path, "wb") as f:
            pickle.dump(_references(), f)
        got = {}
        for value in (None, "0", "2"):   # one child at a time; the first failure ends the test
            got[value] = g = _run(value, path)
            print("SPP_LM_STREAM=%s" % value, {k: "S %.3f xl %.3f xc %.3f g %d" % (v["ratio_S"], v["ratio_xl"], v["ratio_xc"], v["bs_groups"])
                                              for k, v in g.items() if k != "__shards__"})
        for value, form in ((None, 1), ("0", 0), ("2", 2)):   # the kernels each child really launched, and the plan's groups
            for name in CASES:
                assert got[value][name]["lm_stream"] == (0 if name.endswith("32") else form), (value, name)
                assert got[value][name]["bs_groups"] == BS_GROUPS.get(name, got[value][name]["bs_groups"]), (value, name)
        for value in ("0", "2"):
            for name in CASES:
                assert got[value][name]["S"] == got[None][name]["S"], (value, name, "S | rhs differs from the default's")
                assert got[value][name]["x"] == got[None][name]["x"], (value, name, "x differs from the default's")
            assert got[value]["__shards__"] == got[None]["__shards__"], (value, "two shards: packed sum or x differs")
