"""ctypes binding of libspp_hip.so (include/spp_hip.h) plus a host-side mirror of the reference's
linear-solver concept.

`CLinearSolver_HIP` mirrors the duck-typed interface every SLAM++ linear solver implements
(reference include/slam/LinearSolverTags.h:38-135, include/slam/LinearSolver_UberBlock.h:44-427):
same method names, same argument meaning (Lambda upper block triangle + eta overwritten by the
solution), same error behaviour (False = not positive definite, exceptions for everything else).
The C++ twin for linking into the reference itself is include/spp_adapter.h.

There is no CPU fallback here: if the HIP library or a GPU is missing, construction raises.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SPP_LIB") or os.path.join(_HERE, "libspp_hip.so")  # SPP_LIB: another build of the library (A/B experiments)

SPP_OK, SPP_NOT_POSDEF = 0, 1
MODE_AUTO, MODE_SPARSE, MODE_SCHUR, MODE_SCHUR_SPARSE, MODE_SCHUR_MIS = 0, 1, 2, 3, 4
FLAG_PROFILE = 1
INFO = dict(MODE=0, N=1, NNZB=2, NVALS=3, FACTOR_NNZ=4, FACTOR_FLOPS=5, N_REDUCED=6, N_POSES=7,
            N_LANDMARKS=8, SCHUR_PAIRS=9, N_OBS=10, SOLVE_BYTES=11, N_SUPERNODES=12, N_LEVELS=13, S_LD=14, S_NNZB=15, DENSE_STREAMED=16,
            LM_STREAM=17, BS_GROUPS=18, SCHUR_SIDE=19, S_CLEAR=20, S_DEVICE_PTR=21, ASM_HUB_CHUNK=22, SOLVE_ASYNC=23, FACTOR_KEPT=24,
            SPARSE_FACTOR_KEPT=25, SCHUR_SPARSE_FACTOR_KEPT=26)
PHASES = ["permute", "schur_inv", "schur_gemm", "schur_rhs", "factor", "trisolve", "backsubst", "assemble", "total"]

# every symbol include/spp_hip.h declares (tests/test_abi.py checks the .so exports them all)
EXPORTS = [
    "spp_create", "spp_destroy", "spp_free_memory", "spp_last_error", "spp_host_staging", "spp_set_stream", "spp_synchronize",
    "spp_analyze", "spp_set_shard", "spp_get_info", "spp_get_ordering", "spp_sparse_fronts", "spp_factor_solve",
    "spp_factor_solve_device", "spp_solve_device", "spp_marginals_device", "spp_sparse_solve_device", "spp_sparse_marginals_device", "spp_sparse_sigma_device",
    "spp_schur_sigma_device", "spp_dense_potri", "spp_schur_sigma_dense_device",
    "spp_schur_sparse_solve_device", "spp_schur_sparse_marginals_device", "spp_schur_sparse_sigma_device",
    "spp_schur_sparse_sigma_inverse_device",
    "spp_schur_buffer_size", "spp_schur_form", "spp_schur_finish",
    "spp_schur_packed_size", "spp_schur_pack", "spp_schur_unpack",
    "spp_assemble_analyze", "spp_assemble_get_structure", "spp_assemble_device", "spp_assemble_set_edge_weights",
    "spp_assemble_analyze_groups", "spp_assemble_groups_device", "spp_assemble_set_group_edge_weights",
    "spp_assemble_analyze_ternary", "spp_assemble_ternary_device", "spp_ba_intrinsics_linearize_device",
    "spp_ba_intrinsics_update_device",
    "spp_se2_linearize_at_device", "spp_se2_rb_linearize_device", "spp_slam2d_update_device",
    "spp_se3_linearize_at_device", "spp_se3_xyz_linearize_device", "spp_slam3d_update_device", "spp_rocv_range_linearize_device",
    "spp_rocv_cv_linearize_device", "spp_device_malloc",
    "spp_device_free", "spp_memcpy_h2d", "spp_memcpy_d2h", "spp_memcpy_d2d", "spp_get_phase_ms", "spp_get_dominant_kernel",
    "spp_microbench_copy", "spp_microbench_mfma_f64", "spp_microbench_ctile", "spp_microbench_update", "spp_block_ordering", "spp_schur_plan_host", "spp_set_profiling", "spp_se2_linearize_device", "spp_se2_update_device", "spp_ba_linearize_device", "spp_ba_stereo_linearize_device", "spp_ba_update_device", "spp_sim3_ba_linearize_device", "spp_sim3_update_device", "spp_se3_linearize_device", "spp_se3_update_device", "spp_edge_chi2_device", "spp_edge_robust_weights_device", "spp_edge_hessian_maxdiag_device",
    "spp_lm_gain_denominator_device", "spp_dense_potrf_upper", "spp_dense_posv", "spp_dense_posv_multi",
    "spp_dense_posv_masked", "spp_tile_mask_host", "spp_schur_tile_mask_host", "spp_tail_order_host", "spp_tail_plan_host", "spp_schur_cam_order_host",
    "spp_dense_posv_ordered", "spp_tail_step_order_host", "spp_schur_step_order_host",
    "spp_dense_gemm_tn_sub", "spp_dense_gemm_tn_sub_upper", "spp_dense_front_factor", "spp_version",
]

_lib = None
_c_i64p = ctypes.POINTER(ctypes.c_int64)
_c_i32p = ctypes.POINTER(ctypes.c_int32)
_c_f64p = ctypes.POINTER(ctypes.c_double)


class SppError(RuntimeError):
    """std::runtime_error of the C++ adapter (reference LinearSolver_Schur_GPU.cpp:734-797)."""


def load_library():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SppError("libspp_hip.so is not built: run `python -m slam_plus_plus_amd.build` "
                       "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    lib = ctypes.CDLL(LIB_PATH)
    vp, i64, i32, dbl, cint = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_double, ctypes.c_int
    sig = {
        "spp_create": (vp, [cint, cint]),
        "spp_destroy": (None, [vp]),
        "spp_free_memory": (cint, [vp]),
        "spp_last_error": (cint, [vp, ctypes.c_char_p, ctypes.c_size_t]),
        "spp_host_staging": (vp, [vp, i64]),
        "spp_set_stream": (cint, [vp, vp]),
        "spp_synchronize": (cint, [vp]),
        "spp_analyze": (cint, [vp, i64, vp, vp, vp, vp, cint]),
        "spp_set_shard": (cint, [vp, cint, cint]),
        "spp_get_info": (cint, [vp, cint, _c_i64p]),
        "spp_get_ordering": (cint, [vp, vp]),
        "spp_sparse_fronts": (i64, [vp, i64, vp, vp, vp, vp, vp, vp, vp]),
        "spp_factor_solve": (cint, [vp, vp, vp]),
        "spp_factor_solve_device": (cint, [vp, vp, vp]),
        "spp_solve_device": (cint, [vp, vp, vp, i64, i64]),
        "spp_marginals_device": (cint, [vp, vp, i64, vp, vp]),
        "spp_sparse_solve_device": (cint, [vp, vp, i64, i64]),
        "spp_sparse_marginals_device": (cint, [vp, i64, vp, vp]),
        "spp_sparse_sigma_device": (cint, [vp, vp]),
        "spp_schur_sigma_device": (cint, [vp, vp, vp]),
        "spp_schur_sigma_dense_device": (cint, [vp]),
        "spp_schur_sparse_solve_device": (cint, [vp, vp, vp, i64, i64]),
        "spp_schur_sparse_marginals_device": (cint, [vp, vp, i64, vp, vp]),
        "spp_schur_sparse_sigma_device": (cint, [vp, vp, vp]),
        "spp_schur_sparse_sigma_inverse_device": (cint, [vp]),
        "spp_dense_potri": (cint, [vp, vp, i64, i64, vp, i64]),
        "spp_schur_buffer_size": (cint, [vp, _c_i64p]),
        "spp_schur_form": (cint, [vp, vp, vp, vp]),
        "spp_schur_finish": (cint, [vp, vp, vp, vp]),
        "spp_schur_packed_size": (cint, [vp, _c_i64p]),
        "spp_schur_pack": (cint, [vp, vp, vp]),
        "spp_schur_unpack": (cint, [vp, vp, vp]),
        "spp_assemble_analyze": (cint, [vp, i64, vp, i64, vp, vp, cint, cint, cint, i64]),
        "spp_assemble_get_structure": (cint, [vp, vp, vp, vp]),
        "spp_assemble_device": (cint, [vp, vp, vp, vp, vp, dbl, vp, vp]),
        "spp_assemble_set_edge_weights": (cint, [vp, vp]),
        "spp_assemble_analyze_groups": (cint, [vp, i64, vp, cint, vp, vp, vp, vp, vp, vp, vp, i64]),
        "spp_assemble_groups_device": (cint, [vp, vp, vp, vp, vp, dbl, vp, vp]),
        "spp_assemble_set_group_edge_weights": (cint, [vp, cint, vp]),
        "spp_assemble_analyze_ternary": (cint, [vp, i64, vp, i64, vp, vp, vp, cint, cint, cint, cint, cint, i64]),
        "spp_assemble_ternary_device": (cint, [vp, vp, vp, vp, vp, vp, dbl, vp, vp]),
        "spp_ba_intrinsics_linearize_device": (cint, [vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "spp_ba_intrinsics_update_device": (cint, [vp, i64, vp, vp, vp, cint, _c_f64p]),
        "spp_se2_linearize_at_device": (cint, [vp, i64, vp, vp, vp, vp, vp, vp, vp]),
        "spp_se2_rb_linearize_device": (cint, [vp, i64, vp, vp, vp, vp, vp, vp, vp]),
        "spp_slam2d_update_device": (cint, [vp, i64, vp, vp, i64, vp, cint, _c_f64p]),
        "spp_se3_linearize_at_device": (cint, [vp, i64, vp, vp, vp, vp, vp, vp, vp]),
        "spp_se3_xyz_linearize_device": (cint, [vp, i64, vp, vp, vp, vp, vp, vp, vp]),
        "spp_slam3d_update_device": (cint, [vp, i64, vp, vp, i64, vp, cint, _c_f64p]),
        "spp_rocv_range_linearize_device": (cint, [vp, i64, vp, vp, vp, vp, vp, vp, vp]),
        "spp_rocv_cv_linearize_device": (cint, [vp, i64, vp, vp, vp, vp, vp, vp, vp]),
        "spp_device_malloc": (cint, [vp, ctypes.c_size_t, ctypes.POINTER(vp)]),
        "spp_device_free": (cint, [vp, vp]),
        "spp_memcpy_h2d": (cint, [vp, vp, vp, ctypes.c_size_t]),
        "spp_memcpy_d2h": (cint, [vp, vp, vp, ctypes.c_size_t]),
        "spp_memcpy_d2d": (cint, [vp, vp, vp, ctypes.c_size_t]),
        "spp_get_phase_ms": (cint, [vp, _c_f64p]),
        "spp_get_dominant_kernel": (cint, [vp, _c_f64p, _c_i64p, _c_f64p]),
        "spp_microbench_copy": (cint, [vp, ctypes.c_size_t, cint, _c_f64p]),
        "spp_microbench_mfma_f64": (cint, [vp, cint, _c_f64p]),
        "spp_microbench_ctile": (cint, [vp, cint, cint, _c_f64p]),
        "spp_microbench_update": (cint, [vp, ctypes.c_int64, cint, _c_f64p]),
        "spp_block_ordering": (cint, [ctypes.c_int64, vp, vp, cint, vp]),
        "spp_schur_plan_host": (cint, [ctypes.c_int64, vp, vp, vp, cint, cint, cint, vp, vp]),
        "spp_set_profiling": (cint, [vp, cint]),
        "spp_se2_linearize_device": (cint, [vp, ctypes.c_int64, vp, vp, vp, vp, vp, vp, vp]),
        "spp_se2_update_device": (cint, [vp, ctypes.c_int64, vp, vp, cint, _c_f64p]),
        "spp_se3_linearize_device": (cint, [vp, ctypes.c_int64, vp, vp, vp, vp, vp, vp, vp]),
        "spp_se3_update_device": (cint, [vp, ctypes.c_int64, vp, vp, cint, _c_f64p]),
        "spp_edge_chi2_device": (cint, [vp, ctypes.c_int64, cint, vp, vp, _c_f64p]),
        "spp_edge_robust_weights_device": (cint, [vp, ctypes.c_int64, cint, cint, dbl, dbl, vp, vp]),
        "spp_edge_hessian_maxdiag_device": (cint, [vp, ctypes.c_int64, cint, cint, cint, vp, vp, vp, _c_f64p]),
        "spp_lm_gain_denominator_device": (cint, [vp, ctypes.c_int64, vp, vp, ctypes.c_double, _c_f64p]),
        "spp_ba_linearize_device": (cint, [vp, ctypes.c_int64, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "spp_ba_stereo_linearize_device": (cint, [vp, ctypes.c_int64, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "spp_ba_update_device": (cint, [vp, ctypes.c_int64, vp, vp, ctypes.c_int64, vp, vp, vp, ctypes.c_int64, cint, _c_f64p]),
        "spp_sim3_ba_linearize_device": (cint, [vp, ctypes.c_int64, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "spp_sim3_update_device": (cint, [vp, ctypes.c_int64, vp, vp, ctypes.c_int64, vp, vp, vp, ctypes.c_int64, cint, _c_f64p]),
        "spp_dense_potrf_upper": (cint, [vp, vp, i64, i64]),
        "spp_dense_posv": (cint, [vp, vp, i64, i64, vp]),
        "spp_dense_posv_multi": (cint, [vp, vp, i64, i64, vp, i64, i64]),
        "spp_dense_posv_masked": (cint, [vp, vp, i64, i64, vp, vp, i64]),
        "spp_tile_mask_host": (cint, [i64, cint, i64, vp, vp, cint, cint, vp, vp]),
        "spp_schur_tile_mask_host": (cint, [i64, vp, vp, vp, cint, cint, vp]),
        "spp_tail_order_host": (cint, [i64, cint, vp, i64, cint, cint, dbl, vp, vp]),
        "spp_tail_plan_host": (cint, [i64, cint, vp, i64, vp, i64, cint, cint, cint, cint, dbl, vp, vp, vp, vp]),
        "spp_schur_cam_order_host": (cint, [i64, vp, vp, vp, cint, cint, cint, vp, vp, vp]),
        "spp_dense_posv_ordered": (cint, [vp, vp, i64, i64, vp, vp, i64, vp]),
        "spp_tail_step_order_host": (cint, [i64, vp, i64, vp]),
        "spp_schur_step_order_host": (cint, [i64, vp, vp, vp, cint, cint, cint, vp]),
        "spp_dense_gemm_tn_sub": (cint, [vp, i64, i64, i64, vp, i64, vp, i64, vp, i64]),
        "spp_dense_gemm_tn_sub_upper": (cint, [vp, i64, i64, i64, vp, i64, vp, i64, vp, i64]),
        "spp_dense_front_factor": (cint, [vp, vp, i64, i64, i64, vp]),
        "spp_version": (ctypes.c_char_p, []),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


ORDER_AMD, ORDER_ND = 0, 1


def block_ordering(lam, method=ORDER_AMD):
    """Host-only fill-reducing ordering of a BlockCSC / Structure pattern (spp_block_ordering): the
    counterpart of CMatrixOrdering::p_BlockOrdering, src/slam/OrderingMagic.cpp:701. No GPU needed."""
    lib = load_library()
    col_ptr = np.ascontiguousarray(lam.col_ptr, dtype=np.int64)
    row_idx = np.ascontiguousarray(lam.row_idx, dtype=np.int64)
    out = np.empty(lam.nb, dtype=np.int64)
    code = lib.spp_block_ordering(lam.nb, _ptr(col_ptr), _ptr(row_idx), method, _ptr(out))
    if code != 0:
        raise SppError("spp_block_ordering failed: %d" % code)
    return out


def schur_plan_host(lam, shard_rank=0, shard_world=1, sparse_S=False, mis=False):
    """Host-only symbolic Schur plan of a BlockCSC pattern (spp_schur_plan_host): returns a dict with the list sizes,
    a checksum of the pair / block / item lists (checksum), one of every list and scalar of the plan (checksum_all) and
    the wall clock of the plan. mis: the cut of MODE_SCHUR_MIS (one block width, sparse S).
    No GPU needed."""
    lib = load_library()
    col_ptr = np.ascontiguousarray(lam.col_ptr, dtype=np.int64)
    row_idx = np.ascontiguousarray(lam.row_idx, dtype=np.int64)
    dim = np.ascontiguousarray(lam.dim, dtype=np.int32)
    out = np.zeros(9, dtype=np.int64)
    sec = ctypes.c_double(0.0)
    code = lib.spp_schur_plan_host(lam.nb, _ptr(dim), _ptr(col_ptr), _ptr(row_idx), shard_rank, shard_world,
                                   (1 if sparse_S else 0) | (2 if mis else 0), _ptr(out), ctypes.byref(sec))
    if code != 0:
        raise SppError("spp_schur_plan_host failed: %d" % code)
    keys = ("nc", "nl", "no", "n_pairs", "n_sblk", "n_items", "n_multi", "checksum", "checksum_all")
    d = dict(zip(keys, (int(v) for v in out)))
    d["seconds"] = sec.value
    return d


def tile_mask_host(n, bs, i1, i2, has_rhs=True, fill=True):
    """Host-only tile mask of an n x n matrix of bs x bs blocks (i1[q], i2[q]) in 128 x 128 tiles (spp_tile_mask_host):
    returns (words, updates) -- one uint64 per tile row, bit j = tile (i, j) nonzero, and the rank-128 tile updates of a
    factorization on that pattern. words is empty when the matrix has more than 64 tile columns. No GPU needed."""
    lib = load_library()
    i1 = np.ascontiguousarray(i1, dtype=np.int32)
    i2 = np.ascontiguousarray(i2, dtype=np.int32)
    words = np.zeros(64, dtype=np.uint64)
    upd = ctypes.c_int64(0)
    code = lib.spp_tile_mask_host(n, bs, i1.size, _ptr(i1), _ptr(i2), 1 if has_rhs else 0, 1 if fill else 0, _ptr(words),
                                  ctypes.byref(upd))
    if code < 0:
        raise SppError("spp_tile_mask_host failed: %d" % code)
    return words[:code].copy(), upd.value


def schur_tile_mask_host(lam, shard_rank=0, shard_world=1):
    """Host-only: the filled tile mask the dense Schur plan of a BlockCSC pattern hands to the factorization of S
    (spp_schur_tile_mask_host); empty: every tile. No GPU needed."""
    lib = load_library()
    col_ptr = np.ascontiguousarray(lam.col_ptr, dtype=np.int64)
    row_idx = np.ascontiguousarray(lam.row_idx, dtype=np.int64)
    dim = np.ascontiguousarray(lam.dim, dtype=np.int32)
    words = np.zeros(64, dtype=np.uint64)
    code = lib.spp_schur_tile_mask_host(lam.nb, _ptr(dim), _ptr(col_ptr), _ptr(row_idx), shard_rank, shard_world, _ptr(words))
    if code < 0:
        raise SppError("spp_schur_tile_mask_host failed: %d" % code)
    return words[:code].copy()


def schur_cam_order_host(lam, order=None, sparse_S=False, mis=False, shard_rank=0, shard_world=1):
    """Host-only: the camera order the dense Schur plan of a BlockCSC pattern uses and the tile-DAG cost model behind it
    (spp_schur_cam_order_host); without `order` it is read back from the host plan of landmark shard shard_rank of
    shard_world. Returns (cam_order, used, natural, chosen): cam_order[position] = camera in natural
    numbering, used = it differs from the natural order, natural / chosen = dicts with tiles, updates, path (longest chain of
    diagonal tiles) and cost_us of the two orders. With `order` (a permutation of the cameras) nothing is chosen and
    `chosen` holds the model's figures of that order. No GPU needed."""
    lib = load_library()
    col_ptr = np.ascontiguousarray(lam.col_ptr, dtype=np.int64)
    row_idx = np.ascontiguousarray(lam.row_idx, dtype=np.int64)
    dim = np.ascontiguousarray(lam.dim, dtype=np.int32)
    nc = int((dim == dim.max()).sum()) if not mis else int(dim.size)
    out = np.full(max(nc, 1), -1, dtype=np.int64)   # (the MIS cut keeps fewer poses than blocks: trimmed below)
    fig = np.zeros(8, dtype=np.float64)
    oin = None if order is None else np.ascontiguousarray(order, dtype=np.int64)
    if oin is not None and oin.size != nc:
        raise SppError("schur_cam_order_host: order must list every camera once")
    code = lib.spp_schur_cam_order_host(lam.nb, _ptr(dim), _ptr(col_ptr), _ptr(row_idx), shard_rank, shard_world,
                                        (1 if sparse_S else 0) | (2 if mis else 0),
                                        _ptr(oin) if oin is not None else None, _ptr(out), _ptr(fig))
    if code < 0:
        raise SppError("spp_schur_cam_order_host failed: %d" % code)
    keys = ("tiles", "updates", "path", "cost_us")
    natural = dict(zip(keys, (int(fig[0]), int(fig[1]), int(fig[2]), float(fig[3]))))
    chosen = dict(zip(keys, (int(fig[4]), int(fig[5]), int(fig[6]), float(fig[7]))))
    return out[out >= 0], bool(code), natural, chosen


def tail_order_host(n, words, has_rhs=True, resident=256, early=True, beta=0.0):
    """Host-only: the workgroup -> tile table of the streamed dense factor for an n x n matrix with the filled tile mask
    `words` (empty / None: no mask) on a device that holds `resident` workgroups (spp_tail_order_host). Returns
    (tiles, info): tiles is a list of (i, j) in workgroup order, info a dict with n_early (tiles seated in front),
    r_star (their first tile row; the number of tile rows when there are none), rows_resident (D), live_demand, widest.
    early=3: the table with the leading rows of a trailing run that is too large to be seated whole (what the launch uses
    under a step order, SPP_TAIL_EARLY_LEAD). No GPU needed."""
    lib = load_library()
    words = np.ascontiguousarray(words if words is not None else [], dtype=np.uint64)
    table = np.zeros(64 * 65 // 2 + 64, dtype=np.int32)
    info = np.zeros(5, dtype=np.int32)
    code = lib.spp_tail_order_host(int(n), 1 if has_rhs else 0, _ptr(words) if words.size else None, words.size, int(resident),
                                   int(early), float(beta), _ptr(table), _ptr(info))
    if code < 0:
        raise SppError("spp_tail_order_host failed: %d" % code)
    tiles = [(int(t) >> 16, int(t) & 0xffff) for t in table[:code]]
    return tiles, dict(zip(("n_early", "r_star", "rows_resident", "live_demand", "widest"), (int(v) for v in info)))


TAIL_NO_STEP = 127   # the step list's entry behind the last step
SPP_E_BADARG = -1


def tail_plan_host(n, words, step_order=None, front=0, has_rhs=True, tail_rows=44, resident=256, early=3, beta=0.0, tail_mask=True):
    """Host-only: what the host decides for the streamed launch behind the first `front` tile rows (0: the whole
    factorization) of an n x n matrix with the filled tile mask `words` (None: no mask) and the caller's step order
    `step_order` (None: none), from the function the launch calls (spp_tail_plan_host). tail_rows, early (bit 0
    SPP_TAIL_EARLY, bit 1 SPP_TAIL_EARLY_LEAD), beta and tail_mask are the switches' values. Returns None where the region
    is not one streamed launch, else a dict: rowbits (Tr + 1 ints, [0] the row panel in front), steps (the 72 unpacked
    entries of the step list), tiles (list of (i, j) in workgroup order), info (as tail_order_host). A step order that is
    no permutation raises SppError with code SPP_E_BADARG. No GPU needed."""
    lib = load_library()
    words = np.ascontiguousarray(words if words is not None else [], dtype=np.uint64)
    so = np.ascontiguousarray(step_order if step_order is not None else [], dtype=np.int32)
    rowbits = np.zeros(65, dtype=np.uint64)
    steps = np.zeros(72, dtype=np.int32)
    table = np.zeros(64 * 65 // 2 + 64, dtype=np.int32)
    info = np.zeros(5, dtype=np.int32)
    code = lib.spp_tail_plan_host(int(n), 1 if has_rhs else 0, _ptr(words) if words.size else None, words.size,
                                  _ptr(so) if so.size else None, so.size, int(front), int(tail_rows), int(resident),
                                  int(early) | (0 if tail_mask else 4), float(beta), _ptr(rowbits), _ptr(steps), _ptr(table), _ptr(info))
    if code < 0:
        err = SppError("spp_tail_plan_host failed: %d" % code)
        err.code = code
        raise err
    if code == 0:
        return None
    tr = -(-int(n) // 128) - int(front)
    return {"rowbits": [int(w) for w in rowbits[:tr + 1]], "steps": steps.tolist(),
            "tiles": [(int(t) >> 16, int(t) & 0xffff) for t in table[:code]],
            "info": dict(zip(("n_early", "r_star", "rows_resident", "live_demand", "widest"), (int(v) for v in info)))}


def tail_step_order_host(n, words):
    """Host-only: the depth order of the steps of the streamed dense factor for an n x n matrix with the tile mask `words`
    (one uint64 per tile row; closed under elimination by the call, right-hand side column included): the steps sorted by
    the depth of their diagonal tile in the tile DAG, ties by k (spp_tail_step_order_host). No GPU needed."""
    lib = load_library()
    words = np.ascontiguousarray(words, dtype=np.uint64)
    out = np.zeros(64, dtype=np.int32)
    code = lib.spp_tail_step_order_host(int(n), _ptr(words), words.size, _ptr(out))
    if code < 0:
        raise SppError("spp_tail_step_order_host failed: %d" % code)
    return out[:code].copy()


def schur_step_order_host(lam, sparse_S=False, mis=False, shard_rank=0, shard_world=1):
    """Host-only: the step order the dense Schur plan of a BlockCSC pattern hands to the streamed factor, read back from
    the host plan of landmark shard shard_rank of shard_world (spp_schur_step_order_host): one entry per tile row of S,
    the identity unless the camera order is a dissected one; empty without a tile mask. No GPU needed."""
    lib = load_library()
    col_ptr = np.ascontiguousarray(lam.col_ptr, dtype=np.int64)
    row_idx = np.ascontiguousarray(lam.row_idx, dtype=np.int64)
    dim = np.ascontiguousarray(lam.dim, dtype=np.int32)
    out = np.zeros(64, dtype=np.int32)
    code = lib.spp_schur_step_order_host(lam.nb, _ptr(dim), _ptr(col_ptr), _ptr(row_idx), shard_rank, shard_world,
                                         (1 if sparse_S else 0) | (2 if mis else 0), _ptr(out))
    if code < 0:
        raise SppError("spp_schur_step_order_host failed: %d" % code)
    return out[:code].copy()


class DeviceArray:
    """A raw HBM allocation owned through the C ABI (no torch involved)."""

    def __init__(self, ctx, n, dtype=np.float64):
        self.ctx, self.n, self.dtype = ctx, int(n), np.dtype(dtype)
        p = ctypes.c_void_p()
        ctx._check(ctx.lib.spp_device_malloc(ctx.h, self.n * self.dtype.itemsize, ctypes.byref(p)))
        self.ptr = p.value

    @classmethod
    def from_host(cls, ctx, arr):
        arr = np.ascontiguousarray(arr)
        d = cls(ctx, arr.size, arr.dtype)
        d.upload(arr)
        return d

    def upload(self, arr):
        arr = np.ascontiguousarray(arr, dtype=self.dtype)
        assert arr.size == self.n
        self.ctx._check(self.ctx.lib.spp_memcpy_h2d(self.ctx.h, self.ptr, _ptr(arr), arr.nbytes))

    def download(self):
        out = np.empty(self.n, dtype=self.dtype)
        self.ctx._check(self.ctx.lib.spp_memcpy_d2h(self.ctx.h, _ptr(out), self.ptr, out.nbytes))
        return out

    def copy_from(self, other):
        """asynchronous device-to-device copy on the ctx stream"""
        assert other.n * other.dtype.itemsize <= self.n * self.dtype.itemsize
        self.ctx._check(self.ctx.lib.spp_memcpy_d2d(self.ctx.h, self.ptr, other.ptr, other.n * other.dtype.itemsize))

    def free(self):
        if self.ptr:
            self.ctx.lib.spp_device_free(self.ctx.h, self.ptr)
            self.ptr = None


class Context:
    """Thin object wrapper over spp_ctx."""

    def __init__(self, device=0, flags=0):
        self.lib = load_library()
        self.h = self.lib.spp_create(int(device), int(flags))
        if not self.h:
            raise SppError("spp_create failed: no usable HIP device %d (the solver has no CPU fallback)" % device)

    def close(self):
        if getattr(self, "h", None):
            self.lib.spp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        buf = ctypes.create_string_buffer(1024)
        self.lib.spp_last_error(self.h, buf, 1024)
        return buf.value.decode(errors="replace")

    def _check(self, code):
        if code < 0:
            if code == -2:
                raise MemoryError(self.last_error())
            raise SppError("spp error %d: %s" % (code, self.last_error()))
        return code

    # --- symbolic
    def analyze(self, bcsc, mode=MODE_AUTO):
        self._keep = bcsc
        return self._check(self.lib.spp_analyze(self.h, bcsc.nb, _ptr(bcsc.col_ptr), _ptr(bcsc.row_idx),
                                                 _ptr(bcsc.blk_off), _ptr(bcsc.dim), mode))

    def set_shard(self, rank, world):
        return self._check(self.lib.spp_set_shard(self.h, rank, world))

    def info(self, key):
        out = ctypes.c_int64()
        self._check(self.lib.spp_get_info(self.h, INFO[key], ctypes.byref(out)))
        return out.value

    def ordering(self, nb):
        out = np.empty(nb, dtype=np.int64)
        self._check(self.lib.spp_get_ordering(self.h, _ptr(out)))
        return out

    def sparse_fronts(self):
        """the front table of the sparse plan (spp_sparse_fronts): a dict of int32 arrays h, w, pad, cls, level, parent, team,
        one entry per front in elimination order; empty arrays when the analysis built no sparse plan"""
        keys = ("h", "w", "pad", "cls", "level", "parent", "team")
        ns = self._check(self.lib.spp_sparse_fronts(self.h, 0, None, None, None, None, None, None, None))
        out = {k: np.zeros(ns, dtype=np.int32) for k in keys}
        if ns:
            self._check(self.lib.spp_sparse_fronts(self.h, ns, *[_ptr(out[k]) for k in keys]))
        return out

    def se2_linearize_device(self, n_edges, d_v0, d_v1, d_poses, d_meas, d_J0, d_J1, d_r):
        return self._check(self.lib.spp_se2_linearize_device(self.h, n_edges, d_v0, d_v1, d_poses, d_meas, d_J0, d_J1, d_r))

    def se2_update_device(self, n_vertices, d_poses, d_dx, apply=True):
        """returns ||dx|| (host), applies x <- x (+) dx on the device when `apply`"""
        out = ctypes.c_double()
        self._check(self.lib.spp_se2_update_device(self.h, n_vertices, d_poses, d_dx, 1 if apply else 0, ctypes.byref(out)))
        return out.value ** 0.5

    def se2_linearize_at_device(self, n_edges, d_off0, d_off1, d_state, d_meas, d_J0, d_J1, d_r):
        """se2_linearize_device with the poses at scalar offsets (int64) into one flat state"""
        return self._check(self.lib.spp_se2_linearize_at_device(self.h, n_edges, d_off0, d_off1, d_state, d_meas, d_J0, d_J1, d_r))

    def se2_rb_linearize_device(self, n_edges, d_pose_off, d_lm_off, d_state, d_meas, d_J0, d_J1, d_r):
        """range-bearing observations (CEdgePoseLandmark2D): the (3, 2, 2) group's J0, J1, r"""
        return self._check(self.lib.spp_se2_rb_linearize_device(self.h, n_edges, d_pose_off, d_lm_off, d_state, d_meas, d_J0, d_J1, d_r))

    def slam2d_update_device(self, n, d_state, d_dx, n_pose_angles, d_angle_off, apply=True):
        """returns ||dx|| (host); when `apply`, state += dx with the pose angles at d_angle_off clamped"""
        out = ctypes.c_double()
        self._check(self.lib.spp_slam2d_update_device(self.h, n, d_state, d_dx, n_pose_angles, d_angle_off, 1 if apply else 0,
                                                      ctypes.byref(out)))
        return out.value ** 0.5

    def se3_linearize_at_device(self, n_edges, d_off0, d_off1, d_state, d_meas, d_J0, d_J1, d_r):
        """se3_linearize_device with the poses at scalar offsets (int64) into one flat state"""
        return self._check(self.lib.spp_se3_linearize_at_device(self.h, n_edges, d_off0, d_off1, d_state, d_meas, d_J0, d_J1, d_r))

    def se3_xyz_linearize_device(self, n_edges, d_pose_off, d_lm_off, d_state, d_meas, d_J0, d_J1, d_r):
        """XYZ observations of a landmark from a 6D pose (CEdgePoseLandmark3D): the (6, 3, 3) group's J0, J1, r"""
        return self._check(self.lib.spp_se3_xyz_linearize_device(self.h, n_edges, d_pose_off, d_lm_off, d_state, d_meas, d_J0, d_J1, d_r))

    def slam3d_update_device(self, n, d_state, d_dx, n_poses, d_pose_off, apply=True):
        """returns ||dx|| (host); when `apply`, the poses at d_pose_off are composed with their increment, the rest added"""
        out = ctypes.c_double()
        self._check(self.lib.spp_slam3d_update_device(self.h, n, d_state, d_dx, n_poses, d_pose_off, 1 if apply else 0,
                                                      ctypes.byref(out)))
        return out.value ** 0.5

    def rocv_range_linearize_device(self, n_edges, d_recv_off, d_lm_off, d_state, d_meas, d_J0, d_J1, d_r):
        """ranges from a position-velocity receiver to a transmitter (CEdgePosVel_Landmark3D): the (6, 3, 1) group's J0, J1, r"""
        return self._check(self.lib.spp_rocv_range_linearize_device(self.h, n_edges, d_recv_off, d_lm_off, d_state, d_meas, d_J0, d_J1, d_r))

    def rocv_cv_linearize_device(self, n_edges, d_off0, d_off1, d_state, d_dt, d_J0, d_J1, d_r):
        """constant-velocity edges between receivers (CEdgeConstVelocity3D), d_dt the time step of each: a (6, 6, 6) group"""
        return self._check(self.lib.spp_rocv_cv_linearize_device(self.h, n_edges, d_off0, d_off1, d_state, d_dt, d_J0, d_J1, d_r))

    def se3_linearize_device(self, n_edges, d_v0, d_v1, d_poses, d_meas, d_J0, d_J1, d_r):
        return self._check(self.lib.spp_se3_linearize_device(self.h, n_edges, d_v0, d_v1, d_poses, d_meas, d_J0, d_J1, d_r))

    def se3_update_device(self, n_vertices, d_poses, d_dx, apply=True):
        out = ctypes.c_double()
        self._check(self.lib.spp_se3_update_device(self.h, n_vertices, d_poses, d_dx, 1 if apply else 0, ctypes.byref(out)))
        return out.value ** 0.5

    def edge_robust_weights_device(self, n_edges, rd, d_r, d_w, scale, param=1.345, kind=0):
        """w_e = Huber(||r_e|| / scale) on the device (the reference's CRobustify_ErrorNorm_Default with CHuberLossd)"""
        return self._check(self.lib.spp_edge_robust_weights_device(self.h, n_edges, rd, kind, float(scale), float(param), d_r, d_w))

    def edge_chi2_device(self, n_edges, rd, d_r, d_Om):
        out = ctypes.c_double()
        self._check(self.lib.spp_edge_chi2_device(self.h, n_edges, rd, d_r, d_Om, ctypes.byref(out)))
        return out.value

    def edge_hessian_maxdiag_device(self, n_edges, rd, d0, d1, d_J0, d_J1, d_Om):
        out = ctypes.c_double()
        self._check(self.lib.spp_edge_hessian_maxdiag_device(self.h, n_edges, rd, d0, d1, d_J0, d_J1, d_Om, ctypes.byref(out)))
        return out.value

    def lm_gain_denominator_device(self, n, d_dx, d_eta, alpha):
        out = ctypes.c_double()
        self._check(self.lib.spp_lm_gain_denominator_device(self.h, n, d_dx, d_eta, float(alpha), ctypes.byref(out)))
        return out.value

    def ba_linearize_device(self, n_obs, d_cam_of, d_pt_of, d_cams, d_intr, d_points, d_meas, d_J0, d_J1, d_r):
        return self._check(self.lib.spp_ba_linearize_device(self.h, n_obs, d_cam_of, d_pt_of, d_cams, d_intr, d_points,
                                                            d_meas, d_J0, d_J1, d_r))

    def ba_stereo_linearize_device(self, n_obs, d_cam_of, d_pt_of, d_cams, d_intr, d_points, d_meas, d_J0, d_J1, d_r):
        """CEdgeP2SC3D: intr 6 per camera (fx fy cx cy d b), meas 3 per observation (u v u_right); J0 3x6, J1 3x3, r 3"""
        return self._check(self.lib.spp_ba_stereo_linearize_device(self.h, n_obs, d_cam_of, d_pt_of, d_cams, d_intr, d_points,
                                                                   d_meas, d_J0, d_J1, d_r))

    def ba_update_device(self, n_cams, d_cams, d_cam_dxoff, n_points, d_points, d_pt_dxoff, d_dx, n_dx, apply=True):
        out = ctypes.c_double()
        self._check(self.lib.spp_ba_update_device(self.h, n_cams, d_cams, d_cam_dxoff, n_points, d_points, d_pt_dxoff,
                                                  d_dx, n_dx, 1 if apply else 0, ctypes.byref(out)))
        return out.value ** 0.5

    def sim3_ba_linearize_device(self, n_obs, d_cam_of, d_pt_of, d_cams, d_intr, d_points, d_meas, d_J0, d_J1, d_r):
        """CEdgeP2C_XYZ_Sim3_G: cams 7 per camera [t | w | s] in sim(3), intr 5 per camera; J0 2x7, J1 2x3, r 2"""
        return self._check(self.lib.spp_sim3_ba_linearize_device(self.h, n_obs, d_cam_of, d_pt_of, d_cams, d_intr, d_points,
                                                                 d_meas, d_J0, d_J1, d_r))

    def sim3_update_device(self, n_cams, d_cams, d_cam_dxoff, n_points, d_points, d_pt_dxoff, d_dx, n_dx, apply=True):
        """cameras <- Log(Exp(cam) Exp(dx)), points += dx; returns ||dx||"""
        out = ctypes.c_double()
        self._check(self.lib.spp_sim3_update_device(self.h, n_cams, d_cams, d_cam_dxoff, n_points, d_points, d_pt_dxoff,
                                                    d_dx, n_dx, 1 if apply else 0, ctypes.byref(out)))
        return out.value ** 0.5

    def ba_intrinsics_linearize_device(self, n_obs, d_cam_of, d_pt_of, d_intr_of, d_cams, d_intr, d_points, d_meas,
                                       d_J0, d_J1, d_J2, d_r):
        """CEdgeP2CI3D: intr 5 per intrinsics VERTEX (fx fy cx cy kappa), intr_of int32 per observation; J0 2x6, J1 2x3,
        J2 2x6 (last column zeros), r 2"""
        return self._check(self.lib.spp_ba_intrinsics_linearize_device(self.h, n_obs, d_cam_of, d_pt_of, d_intr_of, d_cams,
                                                                       d_intr, d_points, d_meas, d_J0, d_J1, d_J2, d_r))

    def ba_intrinsics_update_device(self, n_intr, d_intr, d_intr_dxoff, d_dx, apply=True):
        """returns ||dx|| over the live coordinates of the intrinsics vertices; when `apply`, CVertexIntrinsics::Operator_Plus"""
        out = ctypes.c_double()
        self._check(self.lib.spp_ba_intrinsics_update_device(self.h, n_intr, d_intr, d_intr_dxoff, d_dx, 1 if apply else 0,
                                                             ctypes.byref(out)))
        return out.value ** 0.5

    def set_profiling(self, on):
        return self._check(self.lib.spp_set_profiling(self.h, 1 if on else 0))

    def set_stream(self, stream_handle):
        return self._check(self.lib.spp_set_stream(self.h, ctypes.c_void_p(stream_handle)))

    def synchronize(self):
        return self._check(self.lib.spp_synchronize(self.h))

    def host_staging(self, n):
        """numpy view of the ctx's page-locked host buffer (spp_host_staging): fill it with the block values and pass
        it to factor_solve() -- the host-pointer entry then copies at the DMA rate of the link"""
        p = self.lib.spp_host_staging(self.h, int(n))
        if not p:
            raise MemoryError(self.last_error())
        return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_double)), shape=(int(n),))

    # --- numeric
    def factor_solve(self, vals, rhs):
        vals = np.ascontiguousarray(vals, dtype=np.float64)
        x = np.array(rhs, dtype=np.float64, copy=True)
        code = self._check(self.lib.spp_factor_solve(self.h, _ptr(vals), _ptr(x)))
        return code, x

    def factor_solve_device(self, d_vals, d_rhs):
        return self._check(self.lib.spp_factor_solve_device(self.h, d_vals, d_rhs))

    def solve_device(self, d_vals, d_B, nrhs, ldb=None):
        """Lambda X = B for nrhs columns (device pointer d_B, column-major, leading dimension ldb, default n) against the
        factor the last successful factor_solve_device left (info("FACTOR_KEPT")); d_vals must be the values that call
        factored. Stream-ordered: B is complete behind synchronize() / a download."""
        if ldb is None:
            ldb = self.info("N")
        return self._check(self.lib.spp_solve_device(self.h, d_vals, d_B, int(ldb), int(nrhs)))

    def _marginals(self, vertices, call):
        """the (m, m) covariance of `vertices`: call(count, vertex pointer, device pointer of the m x m result)"""
        vertices = np.ascontiguousarray(vertices, dtype=np.int64)
        keep = getattr(self, "_keep", None)
        dim = np.asarray(keep.dim) if keep is not None else np.zeros(0, dtype=np.int32)
        if vertices.size == 0 or vertices.min() < 0 or vertices.max() >= dim.size:
            m = 1   # (the library rejects the list; the buffer only has to exist)
        else:
            m = max(1, int(dim[vertices].sum()))
        d_cov = DeviceArray(self, m * m)
        try:
            self._check(call(vertices.size, _ptr(vertices), d_cov.ptr))
            return d_cov.download().reshape((m, m), order="F")
        finally:
            d_cov.free()

    def marginals(self, d_vals, vertices):
        """joint covariance E^T Lambda^-1 E of the given vertices (block columns of Lambda, each at most once, any mix of
        cameras and landmarks) as an (m, m) numpy array, rows and columns in the order of `vertices`; exactly symmetric"""
        return self._marginals(vertices, lambda k, v, cov: self.lib.spp_marginals_device(self.h, d_vals, k, v, cov))

    def sparse_solve_device(self, d_B, nrhs, ldb=None):
        """Lambda X = B for nrhs columns (device pointer d_B, column-major, leading dimension ldb, default n) against the
        sparse factor the last successful factor_solve_device left in MODE_SPARSE (info("SPARSE_FACTOR_KEPT")).
        Stream-ordered: B is complete behind synchronize() / a download."""
        if ldb is None:
            ldb = self.info("N")
        return self._check(self.lib.spp_sparse_solve_device(self.h, d_B, int(ldb), int(nrhs)))

    def sparse_marginals(self, vertices):
        """joint covariance E^T Lambda^-1 E of the given vertices of a pose graph (block columns of Lambda, each at most
        once, any widths and order) from the kept sparse factor, as an (m, m) numpy array; exactly symmetric"""
        return self._marginals(vertices, lambda k, v, cov: self.lib.spp_sparse_marginals_device(self.h, k, v, cov))

    def sparse_sigma_device(self, d_sigma):
        """the blocks of Sigma = Lambda^-1 on the stored pattern of Lambda into d_sigma (device pointer, NVALS doubles in the
        layout of vals) by selected inversion on the kept sparse factor (info("SPARSE_FACTOR_KEPT")). Stream-ordered."""
        return self._check(self.lib.spp_sparse_sigma_device(self.h, d_sigma))

    def sparse_sigma(self):
        """sparse_sigma_device into a host array of NVALS doubles: the block of Sigma at (i, j) where vals holds Lambda's"""
        d_sigma = DeviceArray(self, max(1, self.info("NVALS")))
        try:
            self.sparse_sigma_device(d_sigma.ptr)
            return d_sigma.download()[:self.info("NVALS")]
        finally:
            d_sigma.free()

    def sparse_block_diagonal(self):
        """the diagonal blocks of Sigma = Lambda^-1, one (d_v, d_v) array per vertex v, sliced out of sparse_sigma()
        through blk_off of the analyzed BlockCSC; each exactly symmetric"""
        return self._block_diagonal(self.sparse_sigma())

    def _block_diagonal(self, sigma):
        """the diagonal blocks of a value array in the layout of vals, one per vertex"""
        keep = self._keep
        col_ptr, row_idx, blk_off, dim = (np.asarray(a) for a in (keep.col_ptr, keep.row_idx, keep.blk_off, keep.dim))
        out = []
        for v in range(dim.size):
            p = int(col_ptr[v + 1]) - 1   # (upper incl. diagonal, rows ascending: the diagonal block closes its column)
            assert row_idx[p] == v
            d = int(dim[v])
            out.append(sigma[int(blk_off[p]):int(blk_off[p]) + d * d].reshape((d, d), order="F").copy())
        return out

    def schur_sigma_device(self, d_vals, d_sigma):
        """the blocks of Sigma = Lambda^-1 on the stored pattern of Lambda into d_sigma (device pointer, NVALS doubles in the
        layout of vals) from the kept dense Schur factor (info("FACTOR_KEPT")); d_vals must be the values that factor was
        made from. Stream-ordered."""
        return self._check(self.lib.spp_schur_sigma_device(self.h, d_vals, d_sigma))

    def schur_sigma(self, d_vals):
        """schur_sigma_device into a host array of NVALS doubles: the block of Sigma at (i, j) where vals holds Lambda's"""
        d_sigma = DeviceArray(self, max(1, self.info("NVALS")))
        try:
            self.schur_sigma_device(d_vals, d_sigma.ptr)
            return d_sigma.download()[:self.info("NVALS")]
        finally:
            d_sigma.free()

    def schur_block_diagonal(self, d_vals):
        """the diagonal blocks of Sigma = Lambda^-1 -- a covariance per camera and per point --, one (d_v, d_v) array per
        vertex v, sliced out of schur_sigma() through blk_off of the analyzed BlockCSC; each exactly symmetric"""
        return self._block_diagonal(self.schur_sigma(d_vals))

    def schur_sparse_solve_device(self, d_vals, d_B, nrhs, ldb=None):
        """Lambda X = B for nrhs columns (device pointer d_B, column-major, leading dimension ldb, default n) against the
        factor of the sparse reduced system the last successful factor_solve_device left in MODE_SCHUR_SPARSE
        (info("SCHUR_SPARSE_FACTOR_KEPT")); d_vals must be the values that call factored. Stream-ordered: B is complete
        behind synchronize() / a download."""
        if ldb is None:
            ldb = self.info("N")
        return self._check(self.lib.spp_schur_sparse_solve_device(self.h, d_vals, d_B, int(ldb), int(nrhs)))

    def schur_sparse_marginals(self, d_vals, vertices):
        """joint covariance E^T Lambda^-1 E of the given vertices (block columns of Lambda, each at most once, any mix of
        cameras and landmarks) from the kept factor of the sparse reduced system, as an (m, m) numpy array; exactly symmetric"""
        return self._marginals(vertices, lambda k, v, cov: self.lib.spp_schur_sparse_marginals_device(self.h, d_vals, k, v, cov))

    def schur_sparse_sigma_device(self, d_vals, d_sigma):
        """the blocks of Sigma = Lambda^-1 on the stored pattern of Lambda into d_sigma (device pointer, NVALS doubles in the
        layout of vals) from the kept factor of the sparse reduced system (info("SCHUR_SPARSE_FACTOR_KEPT")); d_vals must be
        the values that factor was made from. Stream-ordered."""
        return self._check(self.lib.spp_schur_sparse_sigma_device(self.h, d_vals, d_sigma))

    def schur_sparse_sigma(self, d_vals):
        """schur_sparse_sigma_device into a host array of NVALS doubles: the block of Sigma at (i, j) where vals holds Lambda's"""
        d_sigma = DeviceArray(self, max(1, self.info("NVALS")))
        try:
            self.schur_sparse_sigma_device(d_vals, d_sigma.ptr)
            return d_sigma.download()[:self.info("NVALS")]
        finally:
            d_sigma.free()

    def schur_sparse_block_diagonal(self, d_vals):
        """the diagonal blocks of Sigma = Lambda^-1 -- a covariance per camera and per point --, one (d_v, d_v) array per
        vertex v, sliced out of schur_sparse_sigma() through blk_off of the analyzed BlockCSC; each exactly symmetric"""
        return self._block_diagonal(self.schur_sparse_sigma(d_vals))

    def dense_potri(self, d_A, n, ld, d_Z, ldz):
        """Z <- A^-1, whole and symmetric, by the dense factor and the block recursion on it (unit tests); returns the status"""
        return self._check(self.lib.spp_dense_potri(self.h, d_A, int(n), int(ld), d_Z, int(ldz)))

    def dense_posv_multi(self, d_A, n, ld, d_B, ldb, nrhs):
        """A X = B for nrhs columns by the dense factor and the multi-column solves (unit tests); returns the status"""
        return self._check(self.lib.spp_dense_posv_multi(self.h, d_A, int(n), int(ld), d_B, int(ldb), int(nrhs)))

    def schur_buffer_size(self):
        out = ctypes.c_int64()
        self._check(self.lib.spp_schur_buffer_size(self.h, ctypes.byref(out)))
        return out.value

    def schur_packed_size(self):
        out = ctypes.c_int64()
        self._check(self.lib.spp_schur_packed_size(self.h, ctypes.byref(out)))
        return out.value

    def schur_pack(self, d_S, d_packed):
        return self._check(self.lib.spp_schur_pack(self.h, d_S, d_packed))

    def schur_unpack(self, d_packed, d_S):
        return self._check(self.lib.spp_schur_unpack(self.h, d_packed, d_S))

    def schur_form(self, d_vals, d_rhs, d_S):
        return self._check(self.lib.spp_schur_form(self.h, d_vals, d_rhs, d_S))

    def schur_finish(self, d_vals, d_S, d_rhs):
        return self._check(self.lib.spp_schur_finish(self.h, d_vals, d_S, d_rhs))

    # --- assembly
    def assemble_analyze(self, dim, v0, v1, d0, d1, rd, unary_vertex=-1):
        dim = np.ascontiguousarray(dim, dtype=np.int32)
        v0 = np.ascontiguousarray(v0, dtype=np.int64)
        v1 = np.ascontiguousarray(v1, dtype=np.int64)
        self._check(self.lib.spp_assemble_analyze(self.h, dim.size, _ptr(dim), v0.size, _ptr(v0), _ptr(v1),
                                                   d0, d1, rd, int(unary_vertex)))
        return self._assemble_structure(dim)

    def _assemble_structure(self, dim):
        nb, nnzb = dim.size, self.info("NNZB")
        col_ptr = np.empty(nb + 1, dtype=np.int64)
        row_idx = np.empty(nnzb, dtype=np.int64)
        blk_off = np.empty(nnzb, dtype=np.int64)
        self._check(self.lib.spp_assemble_get_structure(self.h, _ptr(col_ptr), _ptr(row_idx), _ptr(blk_off)))
        from .blockcsc import BlockCSC
        return BlockCSC(dim, col_ptr, row_idx, blk_off, None, nvals=self.info("NVALS"))

    def assemble_analyze_groups(self, dim, groups, seq=None, unary_vertex=-1):
        """several edge groups in one Lambda. groups: a list of (v0, v1, d0, d1, rd) -- unary edges (priors) as
        (v0, None, d0, 0, rd); seq: None, or per group the global position of each edge (or None). Returns the union
        structure, as assemble_analyze does."""
        dim = np.ascontiguousarray(dim, dtype=np.int32)
        ng = len(groups)
        v0 = [np.ascontiguousarray(g[0], dtype=np.int64) for g in groups]
        v1 = [None if g[1] is None else np.ascontiguousarray(g[1], dtype=np.int64) for g in groups]
        sq = [None if (seq is None or q is None) else np.ascontiguousarray(q, dtype=np.int64) for q in (seq or [None] * ng)]
        parr = lambda arrs: (ctypes.c_void_p * ng)(*[None if a is None else a.ctypes.data for a in arrs])
        ne = np.array([a.size for a in v0], dtype=np.int64)
        d0, d1, rd = (np.array([g[k] for g in groups], dtype=np.int32) for k in (2, 3, 4))
        self._check(self.lib.spp_assemble_analyze_groups(self.h, dim.size, _ptr(dim), ng, _ptr(ne), parr(v0), parr(v1),
                                                          None if seq is None else parr(sq), _ptr(d0), _ptr(d1), _ptr(rd),
                                                          int(unary_vertex)))
        return self._assemble_structure(dim)

    def assemble_analyze_ternary(self, dim, v0, v1, v2, unary_vertex=-1, shape=(6, 3, 6, 2), live2=5):
        """ternary edges (camera v0, point v1, intrinsics v2; the intrinsics vertices 6 wide in dim). Returns the union
        structure, as assemble_analyze does."""
        dim = np.ascontiguousarray(dim, dtype=np.int32)
        v0, v1, v2 = (np.ascontiguousarray(v, dtype=np.int64) for v in (v0, v1, v2))
        self._check(self.lib.spp_assemble_analyze_ternary(self.h, dim.size, _ptr(dim), v0.size, _ptr(v0), _ptr(v1), _ptr(v2),
                                                           shape[0], shape[1], shape[2], live2, shape[3], int(unary_vertex)))
        return self._assemble_structure(dim)

    def assemble_ternary_device(self, d_J0, d_J1, d_J2, d_Om, d_r, damping, d_vals, d_eta):
        return self._check(self.lib.spp_assemble_ternary_device(self.h, d_J0, d_J1, d_J2, d_Om, d_r, float(damping), d_vals, d_eta))

    def assemble_groups_device(self, d_J0, d_J1, d_Om, d_r, damping, d_vals, d_eta):
        """d_J0 ... d_r: one device pointer per group"""
        parr = lambda ptrs: (ctypes.c_void_p * len(ptrs))(*ptrs)
        return self._check(self.lib.spp_assemble_groups_device(self.h, parr(d_J0), parr(d_J1), parr(d_Om), parr(d_r),
                                                               float(damping), d_vals, d_eta))

    def assemble_set_group_edge_weights(self, group, d_w):
        """robust edges of one group: device array of one weight per edge of that group (None: plain edges)"""
        return self._check(self.lib.spp_assemble_set_group_edge_weights(self.h, int(group), d_w))

    def assemble_set_edge_weights(self, d_w):
        """robust edges: device array of one weight per edge for the following assemble_device calls (None: plain edges)"""
        return self._check(self.lib.spp_assemble_set_edge_weights(self.h, d_w))

    def assemble_device(self, d_J0, d_J1, d_Om, d_r, damping, d_vals, d_eta):
        return self._check(self.lib.spp_assemble_device(self.h, d_J0, d_J1, d_Om, d_r, float(damping), d_vals, d_eta))

    # --- profiling
    def phase_ms(self):
        out = np.zeros(len(PHASES))
        self._check(self.lib.spp_get_phase_ms(self.h, out.ctypes.data_as(_c_f64p)))
        return dict(zip(PHASES, out.tolist()))

    def dominant_kernel(self):
        ms, n, fl = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
        self._check(self.lib.spp_get_dominant_kernel(self.h, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl)))
        return ms.value, n.value, fl.value

    def microbench_copy(self, nbytes=1 << 30, iters=10):
        out = ctypes.c_double()
        self._check(self.lib.spp_microbench_copy(self.h, nbytes, iters, ctypes.byref(out)))
        return out.value

    def microbench_ctile(self, n=8192, iters=10):
        out = ctypes.c_double()
        self._check(self.lib.spp_microbench_ctile(self.h, n, iters, ctypes.byref(out)))
        return out.value

    def microbench_update(self, m=5120, iters=20):
        """ms per launch of the stand-alone bulk trailing update of an m x (m + 1) trailing matrix"""
        out = ctypes.c_double()
        self._check(self.lib.spp_microbench_update(self.h, m, iters, ctypes.byref(out)))
        return out.value

    def microbench_mfma_f64(self, iters=4000):
        out = ctypes.c_double()
        self._check(self.lib.spp_microbench_mfma_f64(self.h, iters, ctypes.byref(out)))
        return out.value


class CLinearSolver_HIP:
    """Host-side mirror of the reference's blockwise linear-solver concept.

    reference: typedef CBlockwiseLinearSolverTag _Tag (LinearSolverTags.h:54); the calling sequence
    of CNonlinearSolver_Lambda::Optimize is Clear_SymbolicDecomposition() once, then
    Solve_PosDef_Blocky(lambda, eta) per iteration (NonlinearSolver_Lambda.h:605-626).
    `r_lambda` is a blockcsc.BlockCSC (upper block triangle, values attached), `r_eta` a numpy
    vector that is overwritten with the solution on success and left untouched on failure.
    """
    _Tag = "CBlockwiseLinearSolverTag"

    def __init__(self, device=0, mode=MODE_AUTO, flags=0):
        self._ctx = Context(device, flags)
        self._mode = mode
        self._have_symbolic = False
        self._sig = None

    def Free_Memory(self):
        self._ctx._check(self._ctx.lib.spp_free_memory(self._ctx.h))
        self._have_symbolic = False

    def Clear_SymbolicDecomposition(self):
        self._have_symbolic = False

    def SymbolicDecomposition_Blocky(self, r_lambda):
        self._ctx.analyze(r_lambda, self._mode)
        self._have_symbolic = True
        self._sig = self._signature(r_lambda)
        return True

    @staticmethod
    def _signature(r_lambda):
        """Fingerprint of the block STRUCTURE (not only of its two counts: one edge replaced by another keeps both):
        a 64-bit hash of the column pointers, block rows and block sizes, recomputed on every call (xxh3 runs at memory
        speed: ~5 ms for the 3.4 M blocks of the Venice shape, microseconds for a pose graph). No shortcut through the
        arrays' identities: an array edited in place, or an id recycled after garbage collection, would silently reuse
        a stale symbolic plan (the C++ adapter likewise looks at every block while it flattens)."""
        try:
            import xxhash
            h = xxhash.xxh3_64()
            for a in (r_lambda.col_ptr, r_lambda.row_idx, r_lambda.dim):
                h.update(np.ascontiguousarray(a).view(np.uint8))
            digest = h.intdigest()
        except ImportError:
            import zlib
            digest = 0
            for a in (r_lambda.col_ptr, r_lambda.row_idx, r_lambda.dim):
                digest = zlib.adler32(np.ascontiguousarray(a).view(np.uint8), digest)
        return (r_lambda.nb, r_lambda.nnzb, digest)

    def Solve_PosDef_Blocky(self, r_lambda, r_eta):
        assert r_eta.shape[0] == r_lambda.n, "eta length must equal the matrix dimension"
        if not self._have_symbolic or self._sig is None or self._sig != self._signature(r_lambda):
            self.SymbolicDecomposition_Blocky(r_lambda)
        code, x = self._ctx.factor_solve(r_lambda.vals, r_eta)
        if code == SPP_NOT_POSDEF:
            return False
        r_eta[:] = x
        return True

    def Solve_PosDef(self, r_lambda, r_eta):
        # elementwise entry: symbolic redone on every call (LinearSolver_UberBlock.h:143-258)
        self.Clear_SymbolicDecomposition()
        return self.Solve_PosDef_Blocky(r_lambda, r_eta)

    @property
    def ctx(self):
        return self._ctx
