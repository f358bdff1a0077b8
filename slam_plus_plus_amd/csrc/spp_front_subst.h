// spp_front_subst.h -- substitution on the pivot rows a front keeps (device only): R11^-T t forward and
// R11^-1 (t - R12 t2) backward for up to 16 work columns a workgroup owns, 16 pivots per block. Shared by the solve on the
// kept sparse factor (spp_sparse_solve.hip) and the selected inversion (spp_sparse_sigma.hip,
// section 29); what is deliberately not shared: DESIGN.md section 30.
//
// Front s keeps R[i, c] = F[i + padded(c, w, pad) * ld], i < w, c < h - 1. Two bodies, chosen by the front's size class:
//   classes 0 - 2  fs_lds_fwd / fs_lds_bwd: 256 threads; the caller has staged the pivot rows (fs_stage_rows) and the work
//                  columns T (entry r of column col at T[r * CW + col]) in LDS; every entry is ONE chain of explicit fused
//                  multiply-adds from LDS in a fixed order (pivots ascending forward, columns ascending backward);
//   classes 3 - 4  fs_mfma_fwd / fs_mfma_bwd: 1024 threads, sixteen waves; the products in front of a 16-pivot block are
//                  chains of v_mfma_f64_16x16x4_f64 split over the waves by 16-blocks of the inner index (block b goes to
//                  wave b % 16), each wave ONE chain over its blocks ascending, the partial tiles summed in wave order.
//                  Where the work columns live is the caller's: an accessor type `Cols` answers, for tile column j,
//                      double *piv(p, j)        pivot row p of the column (a column that may not be stored: any address
//                                               inside the caller's memory)
//                      const double *upd(c, j)  row c of the front, w <= c < h - 1, of the column
//                      double start(p, j)       the value pivot row p starts from, or 0
//                      bool may_store(j)        whether the column exists
// In both the diagonal tile is solved by a sweep across 16 lanes per column: the solved pivot goes round by __shfl, every
// later entry takes its product -- entry r still meets its products in the order of the pivots.
// Determinism: which thread and wave sums what depends on the front's shape and the first pivot alone, every sum runs in
// that fixed order, and no sum meets another column's values: a column has the same bits wherever it lands in a tile and
// whatever its neighbours. Operands are masked by an address select in front of the load (a masked lane reads
// fs_zero_word): every lane loads, none outside the front.
// Every thread of the workgroup must call a block loop: they hold barriers.
#pragma once

#include "spp_internal.h"
#include "spp_sparse_plan.h"
#include "spp_tiles.h"

namespace spp {

constexpr int FS_NT = 256;         // threads of a workgroup of the LDS body
constexpr int FS_PB = 16;          // pivots of a block of the triangular solves
constexpr int FS_MT = 1024;        // threads of a workgroup of the MFMA body
constexpr int FS_MW = FS_MT / 64;  // its waves

__device__ const double fs_zero_word = 0.0;

// the 16 x 16 diagonal tile at pivot j0 into LDS (R[i, k] at tri[i + k * 17], upper triangle); beyond the nb valid pivots
// the identity. Masked by address select in front of the load: every lane loads, none outside the front.
__device__ __forceinline__ void fs_stage_tri(const double *F, int ld, int j0, int nb, double *tri)
{
	if(threadIdx.x < FS_PB * FS_PB) {
		const int e = threadIdx.x, i = e & 15, k = e >> 4;
		const bool in = i <= k && k < nb;
		const double v = *(in ? F + (j0 + i) + (int64_t)(j0 + k) * ld : F);
		tri[i + k * 17] = in ? v : (i == k ? 1.0 : 0.0);
	}
}

// forward sweep of the staged tile over the 16 entries of one column held by 16 lanes (R^T y = t): pivot i solved, then
// swept into the rest
__device__ __forceinline__ double fs_sweep_fwd(double t, const double *tri, int r, int lane)
{
#pragma unroll
	for(int i = 0; i < FS_PB; ++ i) {
		const double yi = __shfl(t, (lane & 48) + i) / tri[i + i * 17];
		t = (r == i) ? yi : ((r > i) ? __builtin_fma(-tri[i + r * 17], yi, t) : t);
	}
	return t;
}

// backward sweep (R x = t), from the last pivot up
__device__ __forceinline__ double fs_sweep_bwd(double t, const double *tri, int r, int lane)
{
#pragma unroll
	for(int i = FS_PB - 1; i >= 0; -- i) {
		const double xi = __shfl(t, (lane & 48) + i) / tri[i + i * 17];
		t = (r == i) ? xi : ((r < i) ? __builtin_fma(-tri[r + i * 17], xi, t) : t);
	}
	return t;
}

// ---- classes 0 - 2 ---------------------------------------------------------------------------------------------------
// the w x hc pivot rows of R into LDS: R[i, c] at Rs[i + c * ws]
__device__ __forceinline__ void fs_stage_rows(const double *F, int ld, int w, int pad, int hc, int ws, double *Rs)
{
	for(int e = threadIdx.x; e < w * hc; e += FS_NT) {
		const int i = e % w, c = e / w;
		Rs[i + c * ws] = F[i + (int64_t)padded(c, w, pad) * ld];
	}
}

// behind the product chains of a block (ts[q * CW + col], q < 16): the sweep of the diagonal tile, a lane group of 16 =
// the 16 entries of one column, and the solved pivots back into T. CW < 16 leaves threads without a column.
template <int CW, bool FWD>
__device__ __forceinline__ void fs_lds_sweep(double *T, int j0, int nb, const double *tri, const double *ts)
{
	const int tid = threadIdx.x;
	__syncthreads();
	if(tid < FS_PB * CW) {
		const int r = tid & 15, cc = tid >> 4;
		const double t = FWD ? fs_sweep_fwd(ts[r * CW + cc], tri, r, tid & 63) : fs_sweep_bwd(ts[r * CW + cc], tri, r, tid & 63);
		if(r < nb)
			T[(j0 + r) * CW + cc] = t;
	}
	__syncthreads();
}

// y = R11^-T t in place on T, from pivot p_first (a multiple of 16; the rows above it are zero and take no part) on: per
// block the products with the blocks above, then the diagonal tile
template <int CW>
__device__ __forceinline__ void fs_lds_fwd(const double *Rs, int ws, int w, int p_first, double *T, double *tri, double *ts)
{
	const int col = threadIdx.x % CW, q = threadIdx.x / CW;
	for(int j0 = p_first; j0 < w; j0 += FS_PB) {
		const int nb = (w - j0 < FS_PB) ? w - j0 : FS_PB;
		fs_stage_tri(Rs, ws, j0, nb, tri);
		if(q < FS_PB) {
			double acc = 0.0;
			if(q < nb) {
				const double *Rc = Rs + (j0 + q) * ws;
				acc = T[(j0 + q) * CW + col];
				for(int p = p_first; p < j0; ++ p)
					acc = __builtin_fma(-Rc[p], T[p * CW + col], acc);
			}
			ts[q * CW + col] = acc;
		}
		fs_lds_sweep<CW, true>(T, j0, nb, tri, ts);
	}
}

// x = R11^-1 (y - R12 t) in place on T's pivot rows (t: its rows w .. hc - 1), from the last block up: per block
// everything right of it, then the diagonal tile
template <int CW>
__device__ __forceinline__ void fs_lds_bwd(const double *Rs, int ws, int w, int hc, double *T, double *tri, double *ts)
{
	const int col = threadIdx.x % CW, q = threadIdx.x / CW;
	for(int j0 = ((w - 1) / FS_PB) * FS_PB; j0 >= 0; j0 -= FS_PB) {
		const int nb = (w - j0 < FS_PB) ? w - j0 : FS_PB;
		fs_stage_tri(Rs, ws, j0, nb, tri);
		if(q < FS_PB) {
			double acc = 0.0;
			if(q < nb) {
				const double *Rr = Rs + j0 + q;
				acc = T[(j0 + q) * CW + col];
				for(int c = j0 + nb; c < hc; ++ c)
					acc = __builtin_fma(-Rr[c * ws], T[c * CW + col], acc);
			}
			ts[q * CW + col] = acc;
		}
		fs_lds_sweep<CW, false>(T, j0, nb, tri, ts);
	}
}

// ---- classes 3 - 4 ---------------------------------------------------------------------------------------------------
// D[i][j] += sum over 16 inner indices of A[k][i] B[k][j]; the lane holds A[4 kk + l4][l15], B[4 kk + l4][l15] and
// D[l4 + 4 r][l15] (the layout of tile_atb, spp_tiles.h)
__device__ __forceinline__ v4f64 fs_mfma16(const double *const pa[4], const double *const pb[4], v4f64 acc)
{
	double fa[4], fb[4];
#pragma unroll
	for(int kk = 0; kk < 4; ++ kk) {
		fa[kk] = *pa[kk];
		fb[kk] = *pb[kk];
	}
#pragma unroll
	for(int kk = 0; kk < 4; ++ kk)
		acc = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[kk], fb[kk], acc, 0, 0, 0);
	return acc;
}

// behind a wave's chain of a block: its partial tile out, the start values minus the partial tiles in wave order, the
// sweep of the diagonal tile (waves 0 - 3: a lane group of 16 = the 16 entries of one column) and the store
template <bool FWD, class Cols>
__device__ __forceinline__ void fs_mfma_sweep(const Cols &cols, v4f64 acc, int j0, int nb, const double *tri, double *ts,
	double (*part)[FS_PB * 16])
{
	constexpr int CW = 16;
	const int tid = threadIdx.x, col = tid % CW, q = tid / CW;
	const int lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
#pragma unroll
	for(int r = 0; r < 4; ++ r)
		part[wave][(l4 + 4 * r) * CW + l15] = acc[r];
	__syncthreads();
	if(q < FS_PB) {
		const bool live = q < nb && cols.may_store(col);
		double t = q < nb ? cols.start(j0 + q, col) : 0.0;
#pragma unroll
		for(int v = 0; v < FS_MW; ++ v)
			t -= part[v][q * CW + col];
		ts[q * CW + col] = live ? t : 0.0;
	}
	__syncthreads();
	if(tid < FS_PB * CW) {
		const int r = tid & 15, cc = tid >> 4;
		const double t = FWD ? fs_sweep_fwd(ts[r * CW + cc], tri, r, lane) : fs_sweep_bwd(ts[r * CW + cc], tri, r, lane);
		if(r < nb && cols.may_store(cc))
			*cols.piv(j0 + r, cc) = t;
	}
	__syncthreads();
}

// y = R11^-T t in place on the columns' pivot rows, from pivot p_first (a multiple of 16) on
template <class Cols>
__device__ __forceinline__ void fs_mfma_fwd(const double *F, int ld, int w, int p_first, const Cols &cols, double *tri, double *ts,
	double (*part)[FS_PB * 16])
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;
	for(int j0 = p_first; j0 < w; j0 += FS_PB) {
		const int nb = (w - j0 < FS_PB) ? w - j0 : FS_PB;
		fs_stage_tri(F, ld, j0, nb, tri);
		v4f64 acc = (v4f64){0, 0, 0, 0};
		const bool ci = l15 < nb; // column j0 + l15 of R is a pivot column
		for(int p0 = p_first + wave * FS_PB; p0 < j0; p0 += FS_MW * FS_PB) { // (p0 + 15 < j0 <= w: rows in range)
			const double *pa[4], *pb[4];
#pragma unroll
			for(int kk = 0; kk < 4; ++ kk) {
				const int p = p0 + 4 * kk + l4;
				pa[kk] = ci ? F + p + (int64_t)(j0 + l15) * ld : &fs_zero_word;
				pb[kk] = cols.piv(p, l15);
			}
			acc = fs_mfma16(pa, pb, acc);
		}
		fs_mfma_sweep<true>(cols, acc, j0, nb, tri, ts, part);
	}
}

// x = R11^-1 (y - R12 t) in place on the columns' pivot rows (t: their rows w .. hc - 1), from the last block up
template <class Cols>
__device__ __forceinline__ void fs_mfma_bwd(const double *F, int ld, int w, int pad, int hc, const Cols &cols, double *tri,
	double *ts, double (*part)[FS_PB * 16])
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;
	for(int j0 = ((w - 1) / FS_PB) * FS_PB; j0 >= 0; j0 -= FS_PB) {
		const int nb = (w - j0 < FS_PB) ? w - j0 : FS_PB;
		fs_stage_tri(F, ld, j0, nb, tri);
		v4f64 acc = (v4f64){0, 0, 0, 0};
		const bool ri = l15 < nb; // row j0 + l15 of R is a pivot row
		const double *Fr = F + j0 + l15;
		// the 16-blocks right of the block: n1 inside the pivot columns (from j0 + 16), then n2 beyond (from w); a wave's
		// blocks b ascending through both loops: ONE chain (one loop with the branch inside spilled SGPRs)
		const int n1 = (w - (j0 + nb) + FS_PB - 1) / FS_PB, n2 = (hc - w + FS_PB - 1) / FS_PB;
		int b = wave;
		for(; b < n1; b += FS_MW) {
			const double *pa[4], *pb[4];
#pragma unroll
			for(int kk = 0; kk < 4; ++ kk) {
				const int c = j0 + nb + b * FS_PB + 4 * kk + l4;
				pa[kk] = (ri && c < w) ? Fr + (int64_t)c * ld : &fs_zero_word;
				pb[kk] = c < w ? cols.piv(c, l15) : &fs_zero_word;
			}
			acc = fs_mfma16(pa, pb, acc);
		}
		for(; b < n1 + n2; b += FS_MW) {
			const double *pa[4], *pb[4];
#pragma unroll
			for(int kk = 0; kk < 4; ++ kk) {
				const int c = w + (b - n1) * FS_PB + 4 * kk + l4;
				const bool in = c < hc;
				const double *x = cols.upd(in ? c : w, l15); // (may look the row up: in front of the select, the four side by side)
				pa[kk] = (ri && in) ? Fr + (int64_t)(c + pad) * ld : &fs_zero_word;
				pb[kk] = in ? x : &fs_zero_word;
			}
			acc = fs_mfma16(pa, pb, acc);
		}
		fs_mfma_sweep<false>(cols, acc, j0, nb, tri, ts, part);
	}
}

} // namespace spp
