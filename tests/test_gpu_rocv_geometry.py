"""spp_rocv_range_linearize_device and spp_rocv_cv_linearize_device against the 50-digit cases of tests/rocv_ref.py with the
host test's constants C (|kernel - reference| <= C eps scale), at launch sizes 1, 255, 256, 257 and 65537 bit-identical edge
by edge to the small launch; spp_edge_chi2_device with rd = 1 against the exactly summed reference, with the bound
tests/test_gpu_geometry_scalars.py derives from the kernel's operation order."""
import numpy as np
import pytest

import rocv_ref
from slam_plus_plus_amd import api
from test_gpu_geometry_scalars import EPS, LD, SIZES, _fsum_ld, _passes

pytestmark = pytest.mark.gpu


def _up(ctx, a):
    return api.DeviceArray.from_host(ctx, np.ascontiguousarray(a).ravel())


def _run(ctx, kind, state, off0, off1, meas):
    n = off0.size
    w0, w1, wr = (6, 3, 1) if kind == "rng" else (36, 36, 6)
    lin = ctx.rocv_range_linearize_device if kind == "rng" else ctx.rocv_cv_linearize_device
    d_in = [_up(ctx, a) for a in (off0.astype(np.int64), off1.astype(np.int64), state, meas)]
    d_out = [api.DeviceArray(ctx, w * n) for w in (w0, w1, wr)]
    for d in d_out:
        d.upload(np.full(d.n, np.nan))                    # every entry must be written
    lin(n, d_in[0].ptr, d_in[1].ptr, d_in[2].ptr, d_in[3].ptr, d_out[0].ptr, d_out[1].ptr, d_out[2].ptr)
    out = [d.download().reshape(n, -1) for d in d_out]
    for d in d_in + d_out:
        d.free()
    return out


@pytest.fixture(scope="module")
def small(hip_ctx):
    state, rng_e, cv_e = rocv_ref.cases_as_state()
    return state, {"rng": rng_e, "cv": cv_e}, {k: _run(hip_ctx, k, state, *e) for k, e in (("rng", rng_e), ("cv", cv_e))}


def test_kernels_against_the_50_digit_reference(small):
    _, _, out = small
    J0, J1, r = out["rng"]
    A, B, rc = out["cv"]
    m = A.shape[0]
    got = {"rng_J0": J0, "rng_J1": J1, "rng_r": r[:, 0], "cv_J0": A.reshape(m, 6, 6).transpose(0, 2, 1),
           "cv_J1": B.reshape(m, 6, 6).transpose(0, 2, 1), "cv_r": rc}
    q = rocv_ref.quotients(got)
    print("kernel quotients |kernel - reference| / (eps scale):", {k: round(v, 3) for k, v in q.items()})
    for k, v in q.items():
        assert v <= rocv_ref.C[k], (k, v)
    # e = 0: exact zeros and r = z, nothing divided
    p, l, z = rocv_ref.range_cases()
    assert np.array_equal(l[1], p[1, :3]) and not J0[1].any() and not J1[1].any() and r[1, 0] == z[1]
    assert np.array_equal(J0[:, 3:], np.zeros((z.size, 3))) and np.array_equal(J1, -J0[:, :3])


@pytest.mark.parametrize("kind", ["rng", "cv"])
@pytest.mark.parametrize("n", SIZES)
def test_launch_sizes_give_the_small_launch_bit_for_bit(hip_ctx, small, kind, n):
    state, edges, out = small
    off0, off1, meas = edges[kind]
    pick = (np.arange(n) * 7 + 3) % off0.size
    got = _run(hip_ctx, kind, state, off0[pick], off1[pick], meas[pick])
    for a, b in zip(got, out[kind]):
        assert np.array_equal(a, b[pick])


@pytest.mark.parametrize("n", SIZES)
def test_chi2_of_one_dimensional_residuals(hip_ctx, n):
    rng = np.random.default_rng(100 + n % 97)
    r, Om = rng.normal(size=(n, 1)) * np.exp(rng.normal(size=(n, 1))), rng.uniform(0.5, 400.0, size=(n, 1, 1))
    terms = np.einsum("ei,eij,ej->e", r.astype(LD), Om.astype(LD), r.astype(LD))
    ref, absum = _fsum_ld(terms), float(np.abs(terms).sum())
    dr, dO = _up(hip_ctx, r), _up(hip_ctx, Om)
    got = hip_ctx.edge_chi2_device(n, 1, dr.ptr, dO.ptr)
    assert got == hip_ctx.edge_chi2_device(n, 1, dr.ptr, dO.ptr)
    bound = (2 * 1 + 1 + _passes(n)) * EPS * absum
    print("chi2 rd 1 n %d: |got - exact| = %.3g, bound %.3g" % (n, abs(got - ref), bound))
    assert abs(got - ref) <= bound
    dr.free(), dO.free()
