// spp_schur_dev.h -- device-side pieces of the landmark elimination that more than one translation unit uses
// (spp_schur.hip, spp_solve_again.hip, spp_schur_sigma.hip): the negated inverse of a landmark block and the fetch of a
// pose-landmark block.
#pragma once
#include "spp_internal.h"

namespace spp {

// ---- -(C^-1) of one landmark block (m: DL x DL column-major) ------------------------------------------
template <int DL>
__device__ __forceinline__ void cinv_block(const double *__restrict__ m, double *o)
{
	if(DL == 3) {
		// cofactor formula with ONE reciprocal, determinant expanded along column 0
		// (what Eigen's fixed-size 3x3 inverse evaluates)
#define M_(i, j) m[(i) + 3 * (j)]
#define COF_(i, j) (M_(((i) + 1) % 3, ((j) + 1) % 3) * M_(((i) + 2) % 3, ((j) + 2) % 3) - \
	M_(((i) + 1) % 3, ((j) + 2) % 3) * M_(((i) + 2) % 3, ((j) + 1) % 3))
		const double c00 = COF_(0, 0), c10 = COF_(1, 0), c20 = COF_(2, 0);
		const double det = c00 * M_(0, 0) + c10 * M_(1, 0) + c20 * M_(2, 0);
		const double id = -1.0 / det; // negated: Scale(-1), LinearSolver_Schur.h:1735
		o[0] = c00 * id; o[3] = c10 * id; o[6] = c20 * id;
		o[1] = COF_(0, 1) * id; o[4] = COF_(1, 1) * id; o[7] = COF_(2, 1) * id;
		o[2] = COF_(0, 2) * id; o[5] = COF_(1, 2) * id; o[8] = COF_(2, 2) * id;
#undef COF_
#undef M_
	} else if(DL == 2) {
		const double det = m[0] * m[3] - m[2] * m[1];
		const double id = -1.0 / det;
		o[0] = m[3] * id; o[2] = -m[2] * id;
		o[1] = -m[1] * id; o[3] = m[0] * id;
	} else {
		// 6 x 6 (MIS cut of a 3D pose graph): in-register Gauss-Jordan on [M | I] without pivoting (M is a
		// diagonal block of an SPD matrix); Eigen's general inverse there is an LU with partial pivoting --
		// same result to rounding on SPD blocks
		double a[DL][DL], b[DL][DL];
#pragma unroll
		for(int i = 0; i < DL; ++ i)
#pragma unroll
			for(int j = 0; j < DL; ++ j) {
				a[i][j] = m[i + DL * j];
				b[i][j] = (i == j) ? 1.0 : 0.0;
			}
#pragma unroll
		for(int k = 0; k < DL; ++ k) {
			const double ip = 1.0 / a[k][k];
#pragma unroll
			for(int j = 0; j < DL; ++ j) {
				a[k][j] *= ip;
				b[k][j] *= ip;
			}
#pragma unroll
			for(int i = 0; i < DL; ++ i) {
				if(i == k)
					continue;
				const double f = a[i][k];
#pragma unroll
				for(int j = 0; j < DL; ++ j) {
					a[i][j] -= f * a[k][j];
					b[i][j] -= f * b[k][j];
				}
			}
		}
#pragma unroll
		for(int i = 0; i < DL; ++ i)
#pragma unroll
			for(int j = 0; j < DL; ++ j)
				o[i + DL * j] = -b[i][j];
	}
}

// -(C^-1) of landmark l: stored by the plan (cinv), or formed from the block itself where the plan keeps none
template <int DL>
__device__ __forceinline__ void sa_neg_cinv(const double *__restrict__ cinv, const int64_t *__restrict__ lm_coff,
	const double *__restrict__ vals, int64_t l, double *Ci)
{
	if(cinv) {
#pragma unroll
		for(int e = 0; e < DL * DL; ++ e)
			Ci[e] = cinv[l * DL * DL + e];
	} else
		cinv_block<DL>(vals + lm_coff[l], Ci);
}

// pose-landmark block of Lambda as DP x DL column-major; (offset << 1) | transposed flag
template <int DP, int DL>
__device__ __forceinline__ void load_U(const double *__restrict__ vals, int64_t oo, double *U)
{
	const double *src = vals + (oo >> 1);
	if(oo & 1) { // stored transposed (landmark id < pose id): DL x DP column-major
#pragma unroll
		for(int r = 0; r < DP; ++ r)
#pragma unroll
			for(int q = 0; q < DL; ++ q)
				U[r + DP * q] = src[q + DL * r];
	} else {
#pragma unroll
		for(int e = 0; e < DP * DL; ++ e)
			U[e] = src[e];
	}
}

} // namespace spp
