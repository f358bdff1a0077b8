"""GPU: spp_solve_device and spp_marginals_device on the factor EVERY schedule of the dense Schur path leaves behind.

The two calls never form the factor they use: they read R in the plan's own S buffer (every tile above the diagonal, listed
or not: unlisted tiles must be zero), the whole block inverses in dense.tinv_all and the plan's camera order and lists
(csrc/spp_solve_again.hip, csrc/spp_dense_trsm.h). The switches are read once per process, so every variant below is one
child (tests/solve_again_child.py), run one after the other; the first child that does not exit 0 ends the fixture. Every
child works through sar.SCHEDULE_FIXTURES -- the dissected loops of the three widths (loop63, loop73, loop32), the open chain
in its natural order with unlisted tiles (chain73) and the pair-count spread (edges63) -- with the systems, right-hand sides
and selected vertices this process hands it; no child computes a reference. This process asserts
  liveness   each variant's switches reached its child (the child reports the SPP_* it saw), and where an SPP_INFO word
             reports the switch, the word has the value the existing test of that switch asserts for the factor:
             DENSE_STREAMED (tests/test_gpu_dense_schedules.py, tests/test_gpu_schur_clear.py), S_CLEAR
             (tests/test_gpu_schur_clear.py), LM_STREAM (tests/test_gpu_lm_stream.py), SCHUR_SIDE
             (tests/test_gpu_schur_side.py), SOLVE_ASYNC (tests/test_gpu_solve_async.py), the reported ordering
             (tests/test_gpu_schur_clear.py, tests/test_gpu_solve_async.py).
             Variants WITHOUT a reporting word (only the environment check holds them): SPP_TRSM_FUSED=0,
             SPP_DENSE_SCHED=0, SPP_FUSED=0, SPP_TILE_444=1 and =2, SPP_TAIL_STEP_ORDER=0, SPP_TAIL_EARLY=0,
             SPP_TRSV_CHAIN=0 and =1, SPP_TRSV_MFORM=0, SPP_SACC_FACTORED=0 (with and without SPP_SACC_ULM=0),
             SPP_BACKSUBST_FUSED=0.
  accuracy   every variant, fixture, k and column, with the bounds of tests/test_gpu_solve_again.py and
             tests/test_gpu_marginals.py unchanged: residual ||Lambda x - b|| / ||b|| < 1e-11; error against the refined column
             <= max(1e-10, 4 x the error of the existing path OF THE SAME CHILD on that column); the covariance the same
             against the refined unit columns, exactly symmetric, positive definite diagonal blocks, a vertex alone = its
             block of the joint covariance bit for bit
  bits       in every variant: a repeat, the leading k columns whatever k, a column alone, the NaN frames, x_eta before and
             after, FACTOR_KEPT. SPP_TRSM_FUSED=0 has the default's X and covariance bit for bit; any other variant whose
             x_eta and own S buffer have the default's bits has the default's X too
  sequence   (default child) values A, B, A, a non-positive pivot, B in one context, a 6-column solve behind every good
             factor, both entry points refused behind the bad one; loop73 and then chain73 analyzed in one context: every
             solve equals the same solve of a fresh context.
The reference machinery and the fixtures are checked on the host by tests/test_solve_again_ref_host.py and
tests/test_schur_fixtures_73_host.py."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import schur_side_child as ssc
import solve_again_ref as sar
import test_gpu_dense_schedules as tds
from slam_plus_plus_amd import api

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "solve_again_child.py")

RES_TOL = 1e-11
E_STATE = -5
NAMES = sar.SCHEDULE_FIXTURES
TILE_ROWS = {"loop63": 15, "loop73": 19, "loop32": 8, "chain73": 6, "edges63": 15}
LOOPS = ("loop63", "loop73", "loop32")
MASKED = LOOPS + ("chain73",)          # a tile mask with holes: the clear by listed tiles
STREAM_63 = ("loop63", "edges63")      # 6 x 3 blocks: the widths the streamed landmark kernels are built for
SEQUENCE = ("chain73", "loop73", "loop63")
INFO_WORDS = ("DENSE_STREAMED", "S_CLEAR", "LM_STREAM", "SCHUR_SIDE", "SOLVE_ASYNC", "FACTOR_KEPT", "S_LD", "N_REDUCED", "N_POSES")
ALONE = (0, 15, 16, 127, 128)
VARIANTS = {
    "default": {},
    "trsm0": {"SPP_TRSM_FUSED": "0"},
    "sched0": {"SPP_DENSE_SCHED": "0"},
    "fused0": {"SPP_FUSED": "0"},
    "tile1": {"SPP_TILE_444": "1"},
    "tile2": {"SPP_TILE_444": "2"},
    "la": {"SPP_DENSE_LA": "1"},
    "tail0": {"SPP_DENSE_TAIL": "0"},
    "rows2": {"SPP_TAIL_ROWS": "2"},
    "rows8": {"SPP_TAIL_ROWS": "8"},
    "mask0": {"SPP_TAIL_MASK": "0"},
    "steporder0": {"SPP_TAIL_STEP_ORDER": "0"},
    "early0": {"SPP_TAIL_EARLY": "0"},
    "chain0": {"SPP_TRSV_CHAIN": "0"},
    "chain1": {"SPP_TRSV_CHAIN": "1"},
    "mform0": {"SPP_TRSV_MFORM": "0"},
    "camorder0": {"SPP_SCHUR_CAM_ORDER": "0"},
    "unfactored": {"SPP_SACC_FACTORED": "0"},
    "unfactored_ucm": {"SPP_SACC_FACTORED": "0", "SPP_SACC_ULM": "0"},
    "lmstream0": {"SPP_LM_STREAM": "0"},
    "backsubst0": {"SPP_BACKSUBST_FUSED": "0"},
    "side2": {"SPP_SCHUR_SIDE": "2"},
    "async0": {"SPP_SOLVE_ASYNC": "0"},
}
# tile rows the streamed launch takes of a factorization of t <= 44 tile rows: the table of tests/test_gpu_dense_schedules.py
# as rules (test_each_variant_is_live holds the rules to that table); every variant not named here streams all of them
STREAMED = {"tail0": lambda t: 0, "rows2": lambda t: 2, "rows8": lambda t: min(t, 8), "la": lambda t: t if t <= 5 else 0}
FULL_CLEAR = ("tail0", "mask0")        # tests/test_gpu_schur_clear.py::test_fallback_schedules_force_the_full_clear
TILE_CLEAR = ("default", "camorder0", "side2")   # ...::test_repeated_solves..., test_unlisted_tiles..., test_side_stream...


def selection(name):
    """(vertices shuffled, vertices taken alone): the first camera, a camera of each arc, a separator camera, the camera
    across the first 128-row boundary and two landmarks; without a dissection the first, the middle and the last camera"""
    lam = sar.problem(name)[0]
    dp = int(lam.dim.max())
    nc = int(np.count_nonzero(lam.dim == dp))
    order, used, _, _ = api.schur_cam_order_host(lam)
    straddle = 128 // dp
    assert lam.base[straddle] < 128 < lam.base[straddle + 1] and order[straddle] == straddle
    if used:
        a = int(np.flatnonzero(order != np.arange(nc))[0])            # arc A keeps its natural places
        sep = int(np.flatnonzero(np.diff(order) < 0)[-1]) + 1        # the last drop opens the separators
        assert 0 < a < sep < nc
        cams = [0, int(order[a // 2]), int(order[(a + sep) // 2]), int(order[(sep + nc) // 2]), straddle]
    else:
        cams = [0, nc // 2, nc - 1, straddle]
    sel = cams + [nc + 5, lam.nb - 1]
    assert len(set(sel)) == len(sel)
    return [sel[i] for i in np.random.default_rng(5).permutation(len(sel))], [straddle, lam.nb - 1]


def _child(tmp, tag, env_extra, args):
    out = tmp / (tag + ".npz")
    env = dict(os.environ)
    for k in list(env):
        if k.startswith("SPP_") and k != "SPP_LIB":
            del env[k]
    env.update(env_extra)
    t0 = time.time()
    r = subprocess.run([sys.executable, CHILD, str(tmp / "inputs.npz"), str(out)] + args, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, "%s: exit %d\n%s%s" % (tag, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    print("child %s: %.1f s" % (tag, time.time() - t0))
    return dict(np.load(out))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("solve_again_schedules")
    inputs = {"sequence_names": np.array(SEQUENCE)}
    for name in NAMES:
        lam, eta = sar.problem(name)
        for k in ("dim", "col_ptr", "row_idx", "blk_off", "vals"):
            inputs["%s/%s" % (name, k)] = getattr(lam, k)
        inputs[name + "/eta"] = eta
        inputs[name + "/B"] = sar.rhs_columns(name)
        sel, alone = selection(name)
        inputs[name + "/sel"] = np.array(sel, dtype=np.int64)
        inputs[name + "/sel_alone"] = np.array(alone, dtype=np.int64)
        inputs[name + "/rows"] = sar.vertex_rows(lam, sel)
        if name in SEQUENCE:
            inputs[name + "/vals_b"] = ssc.values_b(lam)
            inputs[name + "/vals_bad"] = ssc.values_bad(lam)
    np.savez(tmp / "inputs.npz", **inputs)
    out = {}
    t0 = time.time()
    for tag, switches in VARIANTS.items():          # one after the other, never side by side
        out[tag] = _child(tmp, tag, switches, [",".join(NAMES)] + (["sequence"] if tag == "default" else []))
    print("%d children: %.1f s" % (len(out), time.time() - t0))
    return out


@pytest.fixture(scope="module")
def cov_refs():
    """name -> (selection, alone, refined covariance, its rows), computed once"""
    refs = {}
    for name in NAMES:
        sel, alone = selection(name)
        cov, _, rows = sar.covariance_ref(name, sel)
        refs[name] = (sel, alone, cov, rows)
    return refs


def _info(res, name, word, which="info"):
    return int(res["%s/%s" % (name, which)][INFO_WORDS.index(word)])


def _pairs(runs):
    for tag in VARIANTS:
        for name in NAMES:
            yield tag, name, runs[tag]


def _ks(name):
    return (1, 6, 17) + ((129,) if sar.rhs_columns(name).shape[1] > 17 else ())


def test_every_variant_ran_every_fixture_and_every_k(runs):
    assert set(runs) == set(VARIANTS) and len(VARIANTS) == 23
    assert _ks("loop32") == (1, 6, 17, 129) and all(_ks(n) == (1, 6, 17) for n in NAMES if n != "loop32")
    for tag, name, res in _pairs(runs):
        want = ["X%d" % k for k in _ks(name)] + ["alone%d" % j for j in ALONE if j < _ks(name)[-1]] + \
            ["base", "base_cov", "x_eta", "x_eta_after", "again", "cov", "cov_again", "frames", "kept", "info", "S_sha", "ordering"]
        missing = [k for k in want if "%s/%s" % (name, k) not in res]
        assert not missing, (tag, name, missing)
        assert res[name + "/base"].shape[1] == _ks(name)[-1], (tag, name, "a column was left out")


def test_each_variant_is_live(runs):
    # the rules of STREAMED against the table of tests/test_gpu_dense_schedules.py (whole factorizations of up to 44 tile rows)
    table = {"default": tds.DEFAULT_PATH}
    table.update({tag: path for tag, _, path, _, _ in tds.VARIANTS})
    steps = [-(-n // 128) for n in tds.SIZES]
    for tag in VARIANTS:
        if tag in table:
            rule = STREAMED.get(tag, lambda t: t)
            assert [rule(t) for t in steps if t <= 44] == [p for t, p in zip(steps, table[tag]) if t <= 44], tag
    for tag, name, res in _pairs(runs):
        T = TILE_ROWS[name]
        nc = _info(res, name, "N_POSES")
        assert sorted(str(s) for s in res["env"]) == sorted("%s=%s" % kv for kv in VARIANTS[tag].items()), (tag, res["env"])
        assert -(-_info(res, name, "N_REDUCED") // 128) == T, (tag, name)
        for which in ("info_first", "info"):
            assert _info(res, name, "DENSE_STREAMED", which) == STREAMED.get(tag, lambda t: t)(T), (tag, name, which, res[name + "/" + which])
            if tag in ("side2", "default"):      # (far below SCHUR_SIDE_MIN_OBS observations: the default is the serial order)
                assert _info(res, name, "SCHUR_SIDE", which) == (1 if tag == "side2" else 0), (tag, name, which)
            if tag in ("async0", "default"):
                assert _info(res, name, "SOLVE_ASYNC", which) == (0 if tag == "async0" else 1), (tag, name, which)
            if tag == "lmstream0":
                assert _info(res, name, "LM_STREAM", which) == 0, (tag, name, which)
            elif tag == "default" and name in STREAM_63:
                assert _info(res, name, "LM_STREAM", which) == 1, (tag, name, which)
        # a new buffer is never cleared by tiles; a repeat is cleared by listed tiles unless the schedule marked the buffer
        assert _info(res, name, "S_CLEAR", "info_first") in (0, 2), (tag, name)
        if name in MASKED and tag in TILE_CLEAR:
            assert _info(res, name, "S_CLEAR") == 1, (tag, name, "the repeat did not clear by listed tiles")
        if name in MASKED and tag in FULL_CLEAR:
            assert _info(res, name, "S_CLEAR") == 0, (tag, name, "the schedule did not mark the buffer")
        natural = np.array_equal(res[name + "/ordering"][:nc], np.arange(nc))
        if tag == "camorder0":
            assert natural, (tag, name, "SPP_SCHUR_CAM_ORDER=0 did not keep the natural order")
        elif tag == "default":
            assert natural == (name not in LOOPS), (tag, name, "the camera order of the loop was not taken" if natural else "reordered")
            assert np.array_equal(res[name + "/ordering"][:nc], api.schur_cam_order_host(sar.problem(name)[0])[0]), (tag, name)


_CSR = {}


def _residuals(name, X, B):
    """per column ||Lambda x - b|| / ||b||, all columns in one sparse product"""
    if name not in _CSR:
        _CSR[name] = sar.problem(name)[0].to_scipy().tocsr()
    return np.linalg.norm(_CSR[name] @ X - B, axis=0) / np.linalg.norm(B, axis=0)


def test_accuracy_of_every_variant(runs):
    worst, worst_res, bad = 0.0, 0.0, []
    for tag, name, res in _pairs(runs):
        lam = sar.problem(name)[0]
        B, Xref = sar.rhs_columns(name), sar.rhs_reference(name)
        e_base = sar.col_err(res[name + "/base"], Xref)
        for k in _ks(name):
            X = res["%s/X%d" % (name, k)]
            assert X.shape == (lam.n, k)
            r = _residuals(name, X, B[:, :k])
            print("%s %s k %d: largest residual %.3e (bound %.0e)" % (tag, name, k, r.max(), RES_TOL))
            worst_res = max(worst_res, float(r.max()))
            if not np.all(r < RES_TOL):
                bad.append((tag, name, k, float(r.max())))
            worst = max(worst, sar.check_criterion(sar.col_err(X, Xref[:, :k]), e_base[:k], "%s %s k %d" % (tag, name, k)))
    print("largest residual over every variant, fixture and k: %.3e (bound %.0e)" % (worst_res, RES_TOL))
    print("largest quotient error / bound over every variant, fixture and k: %.3e" % worst)
    assert not bad, bad


def test_covariances_of_every_variant(runs, cov_refs):
    worst = 0.0
    for tag, name, res in _pairs(runs):
        lam = sar.problem(name)[0]
        sel, alone, cov_ref, rows = cov_refs[name]
        cov = res[name + "/cov"]
        assert cov.shape == (rows.size, rows.size)
        assert np.array_equal(cov, cov.T), (tag, name, "not exactly symmetric")
        worst = max(worst, sar.check_criterion(sar.col_err(cov, cov_ref), sar.col_err(res[name + "/base_cov"], cov_ref),
                                               "%s %s covariance of %d vertices" % (tag, name, len(sel))))
        at = {}
        for v in sel:
            at[v] = sum(int(lam.dim[u]) for u in sel[:sel.index(v)])
            d = int(lam.dim[v])
            np.linalg.cholesky(cov[at[v]:at[v] + d, at[v]:at[v] + d])   # (raises unless positive definite)
        for v in alone:
            d = int(lam.dim[v])
            assert np.array_equal(res["%s/cov_alone%d" % (name, v)], cov[at[v]:at[v] + d, at[v]:at[v] + d]), (tag, name, "vertex %d alone" % v)
        assert np.array_equal(res[name + "/cov_again"], cov), (tag, name, "two runs differ")
    print("largest quotient error / bound over every variant's covariances: %.3e" % worst)


def test_bits_inside_every_variant(runs):
    for tag, name, res in _pairs(runs):
        X = res["%s/X%d" % (name, _ks(name)[-1])]
        assert np.array_equal(res[name + "/again"], X[:, :17]), (tag, name, "two runs differ")
        for k in _ks(name):
            assert np.array_equal(res["%s/X%d" % (name, k)], X[:, :k]), (tag, name, "the leading %d columns depend on k" % k)
        for j in ALONE:
            if j < X.shape[1]:
                assert np.array_equal(res["%s/alone%d" % (name, j)][:, 0], X[:, j]), (tag, name, "column %d depends on its neighbours or its position" % j)
        assert np.all(res[name + "/frames"]), (tag, name, "B was written outside its n rows / k columns")
        assert np.array_equal(res[name + "/x_eta"], res[name + "/x_eta_after"]), (tag, name, "the solves disturbed spp_factor_solve_device")
        assert np.array_equal(res[name + "/x_eta"], res[name + "/base"][:, 0]), (tag, name)
        # FACTOR_KEPT after the analysis, the factor, the solves, the covariances, the last factor
        assert list(res[name + "/kept"]) == [0, 1, 1, 1, 1], (tag, name, res[name + "/kept"])
        assert _info(res, name, "FACTOR_KEPT") == 1
    assert all("loop32/alone128" in res for res in runs.values()), "the two-pass solve did not run"


def _same_x(a, b, name):
    for key in ["X%d" % k for k in _ks(name)] + ["cov"] + ["alone%d" % j for j in ALONE if j < _ks(name)[-1]]:
        if not np.array_equal(a["%s/%s" % (name, key)], b["%s/%s" % (name, key)]):
            return key
    return None


def test_bits_against_the_default(runs):
    """the solve on the kept factor is one code whatever schedule factored: the same factor gives the same X"""
    base = runs["default"]
    for name in NAMES:          # two launches per step or one: the same bits
        assert _same_x(runs["trsm0"], base, name) is None, ("trsm0", name, _same_x(runs["trsm0"], base, name))
    compared = []
    for tag, name, res in _pairs(runs):
        if tag in ("default", "trsm0"):
            continue
        same_factor = np.array_equal(res[name + "/x_eta"], base[name + "/x_eta"]) and np.array_equal(res[name + "/S_sha"], base[name + "/S_sha"])
        if tag == "sched0":     # tests/test_gpu_dense_schedules.py declares R and x of SPP_DENSE_SCHED=0 the default's at every size
            assert same_factor, (tag, name, "x_eta or the S buffer differs from the default's")
        if same_factor:
            compared.append((tag, name))
            assert _same_x(res, base, name) is None, (tag, name, _same_x(res, base, name))
    print("%d (variant, fixture) pairs have the default's x_eta and S buffer and were compared bit for bit: %s" % (len(compared), compared))
    assert all(("sched0", name) in compared for name in NAMES)


def test_one_context_through_other_values_a_failed_pivot_and_another_system(runs):
    res = runs["default"]
    assert [str(s) for s in res["seq/names"]] == list(SEQUENCE)
    for name in SEQUENCE:
        assert res["seq/%s/equal" % name].tolist() == [True] * 4, (name, "A, B, A again, B behind the failed pivot", res["seq/%s/equal" % name])
        assert int(res["seq/%s/bad_code" % name]) == api.SPP_NOT_POSDEF, name
        codes = res["seq/%s/refused" % name]
        assert codes.tolist() == [E_STATE, E_STATE, 1, 0], (name, "return codes, B intact, FACTOR_KEPT", codes)
        # the clears by listed tiles are what is under test: they ran (tests/test_gpu_schur_clear.py)
        assert res["seq/%s/clear" % name][0] in (0, 2) and set(res["seq/%s/clear" % name][1:].tolist()) == {1}, (name, res["seq/%s/clear" % name])
    assert res["seq/analyze/equal"].tolist() == [True, True], "loop73, then chain73 in its buffers"
