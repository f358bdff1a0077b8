// spp_solve_again.hip -- Lambda X = B for k right-hand sides against the factor a dense Schur solve left behind, and the
// joint covariance of chosen vertices on top of it.
//
// After spp_factor_solve_device in the dense Schur mode R (S = R^T R) sits in the plan's own S buffer and the whole block
// inverses in dense.tinv_all; Lambda's values are the caller's. With Lambda = [A U; U^T C] (cameras | landmarks):
//     1  B_l <- C_l^-1 B_l                                       every landmark
//     2  P_c <- B_c - sum_o U_o B_l(o)                            per camera, its observations in cam_obs order
//     3  P   <- S^-1 P                                            dense_potrs_multi (spp_dense_trsm.h); with a sparse reduced
//                                                                 system sparse_solve_again on the kept fronts (section 34)
//     4  B_l <- B_l - C_l^-1 sum_o U_o^T P_c(o)                   per landmark, its observers in lm_ptr order
//     5  B_c <- P_c
// in place on B (n x k in Lambda's row numbering), at most 128 columns per pass through the one camera panel P (ld x 128,
// rows in the plan's camera order). Every sum runs in a fixed order that does not depend on k, with explicit fused
// multiply-adds, and a column never meets another column's values: column j of a k-column solve has the bits of that
// column solved alone. Nothing here writes S, tinv_all, the packed operand or a plan array.

#include "spp_internal.h"
#include "spp_schur_dev.h"

namespace spp {

constexpr int SA_QB = 8; // columns of B a wave (step 2) / a thread (step 4) carries at once: U is fetched once for them

// ---- step 1: one thread per (landmark, group of SA_QB columns): the inverse is formed once for them ----------------------
template <int DL>
__global__ __launch_bounds__(256)
void sa_lm_scale_kernel(int64_t nl, int kc, const int64_t *__restrict__ lm_rbase, const double *__restrict__ cinv,
	const int64_t *__restrict__ lm_coff, const double *__restrict__ vals, double *B, int64_t ldb)
{
	const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const int q0 = (int)blockIdx.y * SA_QB;
	if(l >= nl)
		return;
	double Ci[DL * DL];
	sa_neg_cinv<DL>(cinv, lm_coff, vals, l, Ci);
	double *bl = B + lm_rbase[l];
#pragma unroll
	for(int c = 0; c < SA_QB; ++ c) {
		if(q0 + c < kc) {
			double b[DL];
#pragma unroll
			for(int t = 0; t < DL; ++ t)
				b[t] = bl[t + (int64_t)(q0 + c) * ldb];
#pragma unroll
			for(int t = 0; t < DL; ++ t) {
				double sum = 0;
#pragma unroll
				for(int u = 0; u < DL; ++ u)
					sum = fma(Ci[t + DL * u], b[u], sum);
				bl[t + (int64_t)(q0 + c) * ldb] = -sum; // (Ci is the negated inverse)
			}
		}
	}
}

// ---- step 2: one wave per (camera, group of SA_QB columns); the lanes stride the camera's list, then a butterfly ------
template <int DP, int DL>
__global__ __launch_bounds__(256)
void sa_cam_panel_kernel(int64_t nc, int kc, const int32_t *__restrict__ cam_ptr, const int32_t *__restrict__ cam_obs,
	const int32_t *__restrict__ obs_lm, const int64_t *__restrict__ obs_off, const int64_t *__restrict__ lm_rbase,
	const int64_t *__restrict__ pose_rbase, const double *__restrict__ vals, const double *__restrict__ B, int64_t ldb,
	double *__restrict__ P, int64_t ldp)
{
	const int64_t i = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	const int lane = threadIdx.x & 63, q0 = (int)blockIdx.y * SA_QB;
	if(i >= nc)
		return;
	double s[SA_QB][DP];
#pragma unroll
	for(int c = 0; c < SA_QB; ++ c)
#pragma unroll
		for(int r = 0; r < DP; ++ r)
			s[c][r] = 0;
	for(int32_t p = cam_ptr[i] + lane; p < cam_ptr[i + 1]; p += 64) {
		const int32_t a = cam_obs[p];
		double u[DP * DL];
		load_U<DP, DL>(vals, obs_off[a], u);
		const double *bl = B + lm_rbase[obs_lm[a]];
#pragma unroll
		for(int c = 0; c < SA_QB; ++ c) {
			if(q0 + c < kc) { // (wave-uniform)
#pragma unroll
				for(int t = 0; t < DL; ++ t) {
					const double v = bl[t + (int64_t)(q0 + c) * ldb];
#pragma unroll
					for(int r = 0; r < DP; ++ r)
						s[c][r] = fma(u[r + DP * t], v, s[c][r]);
				}
			}
		}
	}
#pragma unroll
	for(int c = 0; c < SA_QB; ++ c)
#pragma unroll
		for(int r = 0; r < DP; ++ r) {
#pragma unroll
			for(int off = 32; off > 0; off >>= 1)
				s[c][r] += __shfl_xor(s[c][r], off);
		}
	if(lane < DP) {
		const int64_t rb = pose_rbase[i] + lane;
#pragma unroll
		for(int c = 0; c < SA_QB; ++ c) {
			double v = 0;
#pragma unroll
			for(int r = 0; r < DP; ++ r)
				if(lane == r)
					v = s[c][r];
			if(q0 + c < kc)
				P[i * DP + lane + (int64_t)(q0 + c) * ldp] = B[rb + (int64_t)(q0 + c) * ldb] - v;
		}
	}
}

// ---- step 4: one thread per (landmark, group of SA_QB columns), its observers one after the other -------------------
template <int DP, int DL>
__global__ __launch_bounds__(256)
void sa_lm_back_kernel(int64_t nl, int kc, const int32_t *__restrict__ lm_ptr, const int32_t *__restrict__ obs_pose,
	const int64_t *__restrict__ obs_off, const int64_t *__restrict__ lm_rbase, const double *__restrict__ cinv,
	const int64_t *__restrict__ lm_coff, const double *__restrict__ vals, const double *__restrict__ P, int64_t ldp,
	double *B, int64_t ldb)
{
	const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const int q0 = (int)blockIdx.y * SA_QB;
	if(l >= nl)
		return;
	double s[SA_QB][DL];
#pragma unroll
	for(int c = 0; c < SA_QB; ++ c)
#pragma unroll
		for(int t = 0; t < DL; ++ t)
			s[c][t] = 0;
	for(int32_t a = lm_ptr[l]; a < lm_ptr[l + 1]; ++ a) {
		double u[DP * DL];
		load_U<DP, DL>(vals, obs_off[a], u);
		const double *x = P + (int64_t)obs_pose[a] * DP;
#pragma unroll
		for(int c = 0; c < SA_QB; ++ c) {
			if(q0 + c < kc) { // (uniform over the launch's row of workgroups)
#pragma unroll
				for(int r = 0; r < DP; ++ r) {
					const double v = x[r + (int64_t)(q0 + c) * ldp];
#pragma unroll
					for(int t = 0; t < DL; ++ t)
						s[c][t] = fma(u[r + DP * t], v, s[c][t]);
				}
			}
		}
	}
	double Ci[DL * DL];
	sa_neg_cinv<DL>(cinv, lm_coff, vals, l, Ci);
	double *bl = B + lm_rbase[l];
#pragma unroll
	for(int c = 0; c < SA_QB; ++ c) {
		if(q0 + c < kc) {
#pragma unroll
			for(int t = 0; t < DL; ++ t) {
				double sum = 0; // -(C^-1) sum
#pragma unroll
				for(int v = 0; v < DL; ++ v)
					sum = fma(Ci[t + DL * v], s[c][v], sum);
				bl[t + (int64_t)(q0 + c) * ldb] += sum;
			}
		}
	}
}

// ---- step 5: the cameras' solution from the panel (plan order) to their rows of B -------------------------------------
template <int DP>
__global__ __launch_bounds__(256)
void sa_cam_scatter_kernel(int64_t nc, int kc, const int64_t *__restrict__ pose_rbase, const double *__restrict__ P, int64_t ldp,
	double *__restrict__ B, int64_t ldb)
{
	const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const int q = (int)blockIdx.y;
	if(e >= nc * DP || q >= kc)
		return;
	B[pose_rbase[e / DP] + e % DP + (int64_t)q * ldb] = P[e + (int64_t)q * ldp];
}

// `reduced(P, ld, kc)` is step 3 on the camera panel (n_red rows in the plan's camera order, kc <= 128 columns, leading
// dimension ld): dense_potrs_multi on the dense S, sparse_solve_again on the fronts of the sparse one.
template <int DP, int DL, class Reduced>
static void solve_again_t(spp_ctx *ctx, const double *d_vals, double *d_B, int64_t ldb, int64_t nrhs, int64_t ld, const Reduced &reduced)
{
	SchurPlan &sp = ctx->schur;
	hipStream_t s = ctx->stream;
	SPP_REQUIRE(sp.n_red == sp.nc * DP, SPP_E_UNSUPPORTED, "solve on the kept factor: cameras of one width only");
	ctx->again_panel.reserve((size_t)ld * DENSE_NB);
	double *P = ctx->again_panel.p;
	const double *cinv = (sp.factored && DL <= 3) ? (const double*)nullptr : (const double*)sp.cinv.p;
	for(int64_t c0 = 0; c0 < nrhs; c0 += DENSE_NB) {
		const int kc = (int)std::min<int64_t>(DENSE_NB, nrhs - c0);
		const unsigned qg = (unsigned)((kc + SA_QB - 1) / SA_QB);
		double *B = d_B + c0 * ldb;
		if(sp.nl)
			hipLaunchKernelGGL((sa_lm_scale_kernel<DL>), dim3((unsigned)((sp.nl + 255) / 256), qg), dim3(256), 0, s,
				sp.nl, kc, sp.lm_rbase.p, cinv, sp.lm_coff.p, d_vals, B, ldb);
		if(sp.nc) {
			hipLaunchKernelGGL((sa_cam_panel_kernel<DP, DL>), dim3((unsigned)((sp.nc + 3) / 4), qg), dim3(256), 0, s,
				sp.nc, kc, sp.cam_ptr.p, sp.cam_obs.p, sp.obs_lm.p, sp.obs_off.p, sp.lm_rbase.p, sp.pose_rbase.p, d_vals, B, ldb, P, ld);
			reduced(P, ld, kc);
		}
		if(sp.nl && sp.no)
			hipLaunchKernelGGL((sa_lm_back_kernel<DP, DL>), dim3((unsigned)((sp.nl + 255) / 256), qg), dim3(256), 0, s,
				sp.nl, kc, sp.lm_ptr.p, sp.obs_pose.p, sp.obs_off.p, sp.lm_rbase.p, cinv, sp.lm_coff.p, d_vals, P, ld, B, ldb);
		if(sp.nc)
			hipLaunchKernelGGL((sa_cam_scatter_kernel<DP>), dim3((unsigned)((sp.nc * DP + 255) / 256), (unsigned)kc), dim3(256), 0, s,
				sp.nc, kc, sp.pose_rbase.p, P, ld, B, ldb);
	}
	SPP_HIP_CHECK(hipGetLastError());
}

template <class Reduced>
static void solve_again_widths(spp_ctx *ctx, const double *d_vals, double *d_B, int64_t ldb, int64_t nrhs, int64_t ld, const Reduced &reduced)
{
	const int dp = ctx->schur.dp, dl = ctx->schur.dl;
	if(dp == 6 && dl == 3) solve_again_t<6, 3>(ctx, d_vals, d_B, ldb, nrhs, ld, reduced);
	else if(dp == 3 && dl == 2) solve_again_t<3, 2>(ctx, d_vals, d_B, ldb, nrhs, ld, reduced);
	else if(dp == 7 && dl == 3) solve_again_t<7, 3>(ctx, d_vals, d_B, ldb, nrhs, ld, reduced);
	else throw Error(SPP_E_UNSUPPORTED, "solve on the kept factor: block widths not instantiated ({6,3}, {3,2}, {7,3})");
}

void schur_solve_again(spp_ctx *ctx, const double *d_vals, double *d_B, int64_t ldb, int64_t nrhs)
{
	SchurPlan &sp = ctx->schur;
	solve_again_widths(ctx, d_vals, d_B, ldb, nrhs, sp.ld,
		[&](double *P, int64_t ld, int kc) { dense_potrs_multi(ctx, sp.S.p, sp.n_red, ld, P, ld, kc); });
}

// The sparse reduced system: the panel's rows are the numbering of s_st, the matrix the sparse plan
// was made from; sparse_solve_again applies that plan's own permutation inside. Its passes are as wide as this one's.
void schur_sparse_solve_again(spp_ctx *ctx, const double *d_vals, double *d_B, int64_t ldb, int64_t nrhs)
{
	solve_again_widths(ctx, d_vals, d_B, ldb, nrhs, std::max<int64_t>(ctx->schur.n_red, 1),
		[&](double *P, int64_t ld, int kc) { sparse_solve_again(ctx, P, ld, kc); });
}

// ---- covariances ---------------------------------------------------------------------------------------------------
// column j of E is the unit vector of row rows[j]
__global__ __launch_bounds__(256)
void sa_unit_cols_kernel(int64_t m, const int64_t *__restrict__ rows, double *__restrict__ E, int64_t n)
{
	const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(j < m)
		E[rows[j] + j * n] = 1.0;
}

// cov(a, b) = X(rows[a], b) for a <= b, mirrored below: exactly symmetric
__global__ __launch_bounds__(256)
void sa_gather_cov_kernel(int64_t m, const int64_t *__restrict__ rows, const double *__restrict__ X, int64_t n, double *__restrict__ cov)
{
	const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(e >= m * m)
		return;
	const int64_t a = e % m, b = e / m;
	cov[e] = (a <= b) ? X[rows[a] + b * n] : X[rows[b] + a * n];
}

// E^T Lambda^-1 E on either kept factor: the unit columns of the selected rows, `solve` on them, the symmetric gather.
// The whole list is validated first, then the stream is drained, then the host image is rewritten: a refused call
// neither waits nor touches anything.
void kept_marginals(spp_ctx *ctx, const char *who, int64_t n_sel, const int64_t *h_vertices, double *d_cov, const KeptSolve &solve)
{
	const Structure &st = ctx->st;
	hipStream_t s = ctx->stream;
	std::vector<char> seen((size_t)st.nb, 0);
	std::vector<int64_t> rows;
	for(int64_t q = 0; q < n_sel; ++ q) {
		const int64_t v = h_vertices[q];
		SPP_REQUIRE(v >= 0 && v < st.nb, SPP_E_BADARG, std::string(who) + ": vertex out of range");
		SPP_REQUIRE(!seen[(size_t)v], SPP_E_BADARG, std::string(who) + ": a vertex is selected twice");
		seen[(size_t)v] = 1;
		for(int r = 0; r < st.dim[v]; ++ r)
			rows.push_back(st.base[v] + r);
	}
	// (an earlier call's upload of the host image may still be in flight: the stream is drained before it is rewritten)
	SPP_HIP_CHECK(hipStreamSynchronize(s));
	ctx->again_rows_host.swap(rows);
	const int64_t m = (int64_t)ctx->again_rows_host.size(), n = st.n;
	ctx->again_rows.upload(ctx->again_rows_host, s);
	ctx->again_cols.reserve((size_t)n * m);
	SPP_HIP_CHECK(hipMemsetAsync(ctx->again_cols.p, 0, (size_t)n * m * sizeof(double), s));
	hipLaunchKernelGGL(sa_unit_cols_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, m, ctx->again_rows.p, ctx->again_cols.p, n);
	solve(ctx->again_cols.p, n, m);
	hipLaunchKernelGGL(sa_gather_cov_kernel, dim3((unsigned)((m * m + 255) / 256)), dim3(256), 0, s, m, ctx->again_rows.p,
		ctx->again_cols.p, n, d_cov);
	SPP_HIP_CHECK(hipGetLastError());
}

} // namespace spp
