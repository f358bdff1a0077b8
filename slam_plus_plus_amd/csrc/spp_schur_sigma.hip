// spp_schur_sigma.hip -- the blocks of Sigma = Lambda^-1 on the stored pattern of Lambda from the factor a dense Schur
// solve left behind, the job of the reference's CSchurComplement_Marginals::Schur_Marginals
// (include/slam/BAMarginals.h:563-583). The second half of the file does the same from the factor of a SPARSE reduced system.
//
// With Lambda = [A W; W^T C] (cameras | landmarks), S = A - W C^-1 W^T = R^T R and W's blocks the U_o of an observation:
//     1  Z = S^-1, whole and exactly symmetric               dense_potri_upper (spp_dense_potri.h), rows in the plan's camera order
//     2  per landmark l with observers o_1 .. o_k (lm_ptr order, cameras c_i):
//            H_i          = sum_j Z[c_i, c_j] U_j            ss_cross_kernel: eight lanes per (landmark, observer) item
//            Sigma[c_i, l] = -H_i C_l^-1                      ... stored where Lambda stores U_i, transposed where it does
//     3      Sigma[l, l]   = C_l^-1 - C_l^-1 sum_i U_i^T Sigma[c_i, l]     ss_lm_diag_kernel: upper triangle, mirrored
//     4  camera diagonal blocks and stored camera-camera blocks: copies of Z through the plan's camera order (ss_cam_kernel)
// Every double of d_sigma is written exactly once (3 reads what 2 wrote: the launch before it). Every sum runs in an order
// fixed by the lists alone, with explicit fused multiply-adds and a fixed butterfly. Nothing here writes S, tinv_all or a
// plan array; the only state is the workspace Z and the list of camera-camera blocks, made on the first call.

#include "spp_internal.h"
#include "spp_schur_dev.h"

namespace spp {

constexpr int SS_LANES = 8; // lanes that share one (landmark, observer) item: a 256-track is 256 items of 32 steps each

// ---- step 2: the cross blocks ----------------------------------------------------------------------------------------
template <int DP, int DL>
__global__ __launch_bounds__(256)
void ss_cross_kernel(int64_t no, const int32_t *__restrict__ lm_ptr, const int32_t *__restrict__ obs_pose,
	const int32_t *__restrict__ obs_lm, const int64_t *__restrict__ obs_off, const double *__restrict__ cinv,
	const int64_t *__restrict__ lm_coff, const double *__restrict__ vals, const double *__restrict__ Z, int64_t ldz,
	double *__restrict__ sigma)
{
	const int64_t a = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / SS_LANES;
	const int g = threadIdx.x & (SS_LANES - 1);
	if(a >= no) // (a whole group of lanes leaves together)
		return;
	const int32_t l = obs_lm[a];
	const double *zr = Z + (int64_t)obs_pose[a] * DP;
	double h[DP * DL];
#pragma unroll
	for(int e = 0; e < DP * DL; ++ e)
		h[e] = 0;
	for(int32_t b = lm_ptr[l] + g; b < lm_ptr[l + 1]; b += SS_LANES) {
		double u[DP * DL];
		load_U<DP, DL>(vals, obs_off[b], u);
		const double *zb = zr + (int64_t)obs_pose[b] * DP * ldz;
#pragma unroll
		for(int q = 0; q < DP; ++ q)
#pragma unroll
			for(int r = 0; r < DP; ++ r) {
				const double z = zb[r + q * ldz];
#pragma unroll
				for(int t = 0; t < DL; ++ t)
					h[r + DP * t] = fma(z, u[q + DP * t], h[r + DP * t]);
			}
	}
#pragma unroll
	for(int e = 0; e < DP * DL; ++ e) {
#pragma unroll
		for(int off = SS_LANES / 2; off > 0; off >>= 1)
			h[e] += __shfl_xor(h[e], off);
	}
	double Ci[DL * DL]; // -(C^-1)
	sa_neg_cinv<DL>(cinv, lm_coff, vals, l, Ci);
	const int64_t oo = obs_off[a];
	double *dst = sigma + (oo >> 1);
#pragma unroll
	for(int t = 0; t < DL; ++ t)
#pragma unroll
		for(int r = 0; r < DP; ++ r) {
			double x = 0;
#pragma unroll
			for(int v = 0; v < DL; ++ v)
				x = fma(h[r + DP * v], Ci[v + DL * t], x);
			if(((r + DP * t) & (SS_LANES - 1)) == g) // (every lane holds the whole block: the stores are dealt out)
				dst[(oo & 1) ? t + DL * r : r + DP * t] = x;
		}
}

// ---- step 3: one thread per landmark, its observers one after the other -------------------------------------------
// (serial on purpose: this sum has k terms for a landmark of degree k, not the k^2 of step 2 -- 257 steps of 18 fma
// on the longest track of the fixtures, 0.3 ms of a 12 ms call on the Venice shape -- and one thread keeps list order)
template <int DP, int DL>
__global__ __launch_bounds__(256)
void ss_lm_diag_kernel(int64_t nl, const int32_t *__restrict__ lm_ptr, const int64_t *__restrict__ obs_off,
	const double *__restrict__ cinv, const int64_t *__restrict__ lm_coff, const double *__restrict__ vals, double *sigma)
{
	const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(l >= nl)
		return;
	double m[DL * DL]; // sum_i U_i^T Sigma[c_i, l]
#pragma unroll
	for(int e = 0; e < DL * DL; ++ e)
		m[e] = 0;
	for(int32_t a = lm_ptr[l]; a < lm_ptr[l + 1]; ++ a) {
		double u[DP * DL], x[DP * DL];
		load_U<DP, DL>(vals, obs_off[a], u);
		load_U<DP, DL>(sigma, obs_off[a], x);
#pragma unroll
		for(int r = 0; r < DP; ++ r)
#pragma unroll
			for(int t = 0; t < DL; ++ t)
#pragma unroll
				for(int v = 0; v < DL; ++ v)
					m[v + DL * t] = fma(u[r + DP * v], x[r + DP * t], m[v + DL * t]);
	}
	double Ci[DL * DL]; // N = -(C^-1):  Sigma[l, l] = -N + N m
	sa_neg_cinv<DL>(cinv, lm_coff, vals, l, Ci);
	double *dst = sigma + lm_coff[l];
#pragma unroll
	for(int t = 0; t < DL; ++ t)
#pragma unroll
		for(int v = 0; v <= t; ++ v) {
			double s = -Ci[v + DL * t];
#pragma unroll
			for(int w = 0; w < DL; ++ w)
				s = fma(Ci[v + DL * w], m[w + DL * t], s);
			dst[v + DL * t] = s;
			if(v < t)
				dst[t + DL * v] = s;
		}
}

// ---- step 4: the stored camera-camera blocks, diagonal ones included, are blocks of Z -----------------------------
// cc: three words per block -- offset in vals, position of the row camera, position of the column camera
template <int DP>
__global__ __launch_bounds__(256)
void ss_cam_kernel(int64_t ncc, const int64_t *__restrict__ cc, const double *__restrict__ Z, int64_t ldz, double *__restrict__ sigma)
{
	const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(e >= ncc * DP * DP)
		return;
	const int64_t k = e / (DP * DP);
	const int rq = (int)(e % (DP * DP)), r = rq % DP, q = rq / DP;
	sigma[cc[3 * k] + rq] = Z[cc[3 * k + 1] * DP + r + (cc[3 * k + 2] * DP + q) * ldz];
}

// the camera-camera blocks of Lambda's stored pattern with their cameras' positions in the plan's order
static void sigma_cam_blocks(spp_ctx *ctx)
{
	SchurPlan &sp = ctx->schur;
	const Structure &st = ctx->st;
	std::vector<int64_t> pos((size_t)st.nb, -1);
	for(size_t p = 0; p < sp.pose_block.size(); ++ p)
		pos[(size_t)sp.pose_block[p]] = (int64_t)p;
	std::vector<int64_t> &cc = sp.sigma_cc_host;
	cc.clear();
	for(int64_t j = 0; j < st.nb; ++ j) {
		if(pos[(size_t)j] < 0)
			continue;
		for(int64_t p = st.col_ptr[j]; p < st.col_ptr[j + 1]; ++ p) {
			const int64_t i = st.row_idx[p];
			if(pos[(size_t)i] < 0)
				continue;
			cc.push_back(st.blk_off[p]);
			cc.push_back(pos[(size_t)i]);
			cc.push_back(pos[(size_t)j]);
		}
	}
	sp.sigma_ncc = (int64_t)cc.size() / 3;
	sp.sigma_cc.upload(cc, ctx->stream); // (the host image lives in the plan: the copy may still be in flight on return)
}

template <int DP, int DL>
static void schur_sigma_t(spp_ctx *ctx, const double *d_vals, double *d_sigma, bool dense_only)
{
	SchurPlan &sp = ctx->schur;
	hipStream_t s = ctx->stream;
	const int64_t ld = sp.ld;
	SPP_REQUIRE(sp.n_red == sp.nc * DP, SPP_E_UNSUPPORTED, "spp_schur_sigma_device: cameras of one width only");
	sp.sigma_Z.reserve((size_t)ld * ld);
	if(sp.sigma_ncc < 0)
		sigma_cam_blocks(ctx);
	double *Z = sp.sigma_Z.p;
	if(sp.n_red)
		dense_potri_upper(ctx, sp.S.p, sp.n_red, ld, Z, ld);
	if(dense_only)
		return;
	const double *cinv = (sp.factored && DL <= 3) ? (const double*)nullptr : (const double*)sp.cinv.p;
	if(sp.no)
		hipLaunchKernelGGL((ss_cross_kernel<DP, DL>), dim3((unsigned)((sp.no * SS_LANES + 255) / 256)), dim3(256), 0, s,
			sp.no, sp.lm_ptr.p, sp.obs_pose.p, sp.obs_lm.p, sp.obs_off.p, cinv, sp.lm_coff.p, d_vals, Z, ld, d_sigma);
	if(sp.nl)
		hipLaunchKernelGGL((ss_lm_diag_kernel<DP, DL>), dim3((unsigned)((sp.nl + 255) / 256)), dim3(256), 0, s,
			sp.nl, sp.lm_ptr.p, sp.obs_off.p, cinv, sp.lm_coff.p, d_vals, d_sigma);
	if(sp.sigma_ncc)
		hipLaunchKernelGGL((ss_cam_kernel<DP>), dim3((unsigned)((sp.sigma_ncc * DP * DP + 255) / 256)), dim3(256), 0, s,
			sp.sigma_ncc, sp.sigma_cc.p, Z, ld, d_sigma);
	SPP_HIP_CHECK(hipGetLastError());
}

void schur_sigma(spp_ctx *ctx, const double *d_vals, double *d_sigma, bool dense_only)
{
	const int dp = ctx->schur.dp, dl = ctx->schur.dl;
	if(dp == 6 && dl == 3) schur_sigma_t<6, 3>(ctx, d_vals, d_sigma, dense_only);
	else if(dp == 3 && dl == 2) schur_sigma_t<3, 2>(ctx, d_vals, d_sigma, dense_only);
	else if(dp == 7 && dl == 3) schur_sigma_t<7, 3>(ctx, d_vals, d_sigma, dense_only);
	else throw Error(SPP_E_UNSUPPORTED, "spp_schur_sigma_device: block widths not instantiated ({6,3}, {3,2}, {7,3})");
}

// ==== the sparse reduced system ====
// The blocks of Sigma = Lambda^-1 on the stored pattern of Lambda from the factor a Schur
// solve with a SPARSE reduced system left behind: the steps above with Z = S^-1 known on the
// stored pattern of S only.
//
// With Lambda = [A W; W^T C] (cameras | landmarks), S = A - W C^-1 W^T = R^T R in the fronts of the sparse plan:
//     1  Zb = the blocks of Z = S^-1 on the stored pattern of S   selected inversion (sparse_sigma_arena), gathered into a
//                                                                  workspace in the layout of S's value array
//     2  per landmark l with observers o_1 .. o_k (lm_ptr order, cameras c_i):
//            H_i          = sum_j Z[c_i, c_j] U_j                 ssp_cross_kernel: eight lanes per (landmark, observer) item
//            Sigma[c_i, l] = -H_i C_l^-1                           ... stored where Lambda stores U_i, transposed where it does
//     3      Sigma[l, l]   = C_l^-1 - C_l^-1 sum_i U_i^T Sigma[c_i, l]     ss_lm_diag_kernel above, as it is
//     4  camera diagonal blocks and stored camera-camera blocks: copies out of Zb through sblk_voff / sblk_aoff (ssp_cam_kernel)
// Two cameras that share a landmark share a stored block of S, so every Z[c_i, c_j] of step 2 is a block of Zb: the upper
// one, (min, max), read transposed when c_i > c_j. It is found by bisection of the ascending row list of block column
// max(c_i, c_j) of S: O(blocks of S) words of lists instead of a table of one offset per pair.
// Every double of d_sigma is written exactly once (3 reads what 2 wrote: the launch before it). Every sum runs in an order
// fixed by the lists alone, with explicit fused multiply-adds and a fixed butterfly; every dependency is a launch boundary.
// Nothing here writes S's buffer, the fronts, cinv or a plan array.

// ---- step 2: the cross blocks ----------------------------------------------------------------------------------------
template <int DP, int DL>
__global__ __launch_bounds__(256)
void ssp_cross_kernel(int64_t no, const int32_t *__restrict__ lm_ptr, const int32_t *__restrict__ obs_pose,
	const int32_t *__restrict__ obs_lm, const int64_t *__restrict__ obs_off, const double *__restrict__ cinv,
	const int64_t *__restrict__ lm_coff, const double *__restrict__ vals, const int64_t *__restrict__ s_col,
	const int64_t *__restrict__ s_row, const double *__restrict__ Zb, double *__restrict__ sigma)
{
	const int64_t a = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / SS_LANES;
	const int g = threadIdx.x & (SS_LANES - 1);
	if(a >= no) // (a whole group of lanes leaves together)
		return;
	const int32_t l = obs_lm[a];
	const int32_t ca = obs_pose[a];
	double h[DP * DL];
#pragma unroll
	for(int e = 0; e < DP * DL; ++ e)
		h[e] = 0;
	for(int32_t b = lm_ptr[l] + g; b < lm_ptr[l + 1]; b += SS_LANES) {
		double u[DP * DL];
		load_U<DP, DL>(vals, obs_off[b], u);
		const int32_t cb = obs_pose[b];
		const bool tr = ca > cb;
		const int64_t lo = tr ? cb : ca, hi = tr ? ca : cb;
		// the first entry >= lo of column hi's rows: the block (lo, hi) is stored, so that is it (the diagonal block closes
		// the column: the search never leaves it)
		int64_t p0 = s_col[hi], p1 = s_col[hi + 1] - 1;
		while(p0 < p1) {
			const int64_t mid = (p0 + p1) >> 1;
			if(s_row[mid] < lo)
				p0 = mid + 1;
			else
				p1 = mid;
		}
		const double *zb = Zb + p0 * (DP * DP);
		double z[DP * DP];
#pragma unroll
		for(int e = 0; e < DP * DP; ++ e)
			z[e] = zb[e];
#pragma unroll
		for(int q = 0; q < DP; ++ q)
#pragma unroll
			for(int r = 0; r < DP; ++ r) {
				const double zrq = tr ? z[q + DP * r] : z[r + DP * q]; // Z[ca, cb](r, q)
#pragma unroll
				for(int t = 0; t < DL; ++ t)
					h[r + DP * t] = fma(zrq, u[q + DP * t], h[r + DP * t]);
			}
	}
#pragma unroll
	for(int e = 0; e < DP * DL; ++ e) {
#pragma unroll
		for(int off = SS_LANES / 2; off > 0; off >>= 1)
			h[e] += __shfl_xor(h[e], off);
	}
	double Ci[DL * DL]; // -(C^-1)
	sa_neg_cinv<DL>(cinv, lm_coff, vals, l, Ci);
	const int64_t oo = obs_off[a];
	double *dst = sigma + (oo >> 1);
#pragma unroll
	for(int t = 0; t < DL; ++ t)
#pragma unroll
		for(int r = 0; r < DP; ++ r) {
			double x = 0;
#pragma unroll
			for(int v = 0; v < DL; ++ v)
				x = fma(h[r + DP * v], Ci[v + DL * t], x);
			if(((r + DP * t) & (SS_LANES - 1)) == g) // (every lane holds the whole block: the stores are dealt out)
				dst[(oo & 1) ? t + DL * r : r + DP * t] = x;
		}
}

// ---- step 4: the stored camera-camera blocks of Lambda, diagonal ones included, are blocks of Zb -------------------
// a thread per double of a block of S; aoff: the plan's word for the block of A it carries (-1 none, -2 - offset: stored
// transposed)
template <int DP>
__global__ __launch_bounds__(256)
void ssp_cam_kernel(int64_t n_sblk, const int64_t *__restrict__ sblk_voff, const int64_t *__restrict__ sblk_aoff,
	const double *__restrict__ Zb, double *__restrict__ sigma)
{
	const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(e >= n_sblk * DP * DP)
		return;
	const int64_t b = e / (DP * DP), aoff = sblk_aoff[b];
	const int rq = (int)(e % (DP * DP)), r = rq % DP, q = rq / DP;
	if(aoff == -1)
		return;
	const double z = Zb[sblk_voff[b] + rq];
	if(aoff >= 0)
		sigma[aoff + rq] = z;
	else
		sigma[(-2 - aoff) + q + DP * r] = z;
}

template <int DP, int DL>
static void schur_sparse_sigma_t(spp_ctx *ctx, const double *d_vals, double *d_sigma, bool inverse_only)
{
	SchurPlan &sp = ctx->schur;
	hipStream_t s = ctx->stream;
	SPP_REQUIRE(sp.n_red == sp.nc * DP, SPP_E_UNSUPPORTED, "spp_schur_sparse_sigma_device: cameras of one width only");
	SPP_REQUIRE(sp.s_st.nvals == sp.n_sblk * DP * DP && (int64_t)sp.s_st.col_ptr.size() == sp.nc + 1, SPP_E_HIP,
		"internal: the value array of S is not its blocks one after the other");
	if(!sp.sigma_scol.p) { // (the host images live in the plan: the copies may still be in flight on return)
		sp.sigma_scol.upload(sp.s_st.col_ptr, s);
		sp.sigma_srow.upload(sp.s_st.row_idx, s);
		sp.sigma_Zb.reserve((size_t)std::max<int64_t>(sp.s_st.nvals, 1));
	}
	double *Zb = sp.sigma_Zb.p;
	sparse_sigma_arena(ctx);
	sparse_sigma_gather(ctx, Zb);
	if(inverse_only)
		return;
	const double *cinv = (sp.factored && DL <= 3) ? (const double*)nullptr : (const double*)sp.cinv.p;
	if(sp.no)
		hipLaunchKernelGGL((ssp_cross_kernel<DP, DL>), dim3((unsigned)((sp.no * SS_LANES + 255) / 256)), dim3(256), 0, s,
			sp.no, sp.lm_ptr.p, sp.obs_pose.p, sp.obs_lm.p, sp.obs_off.p, cinv, sp.lm_coff.p, d_vals, sp.sigma_scol.p,
			sp.sigma_srow.p, Zb, d_sigma);
	if(sp.nl)
		hipLaunchKernelGGL((ss_lm_diag_kernel<DP, DL>), dim3((unsigned)((sp.nl + 255) / 256)), dim3(256), 0, s,
			sp.nl, sp.lm_ptr.p, sp.obs_off.p, cinv, sp.lm_coff.p, d_vals, d_sigma);
	if(sp.n_sblk)
		hipLaunchKernelGGL((ssp_cam_kernel<DP>), dim3((unsigned)((sp.n_sblk * DP * DP + 255) / 256)), dim3(256), 0, s,
			sp.n_sblk, sp.sblk_voff.p, sp.sblk_aoff.p, Zb, d_sigma);
	SPP_HIP_CHECK(hipGetLastError());
}

void schur_sparse_sigma(spp_ctx *ctx, const double *d_vals, double *d_sigma, bool inverse_only)
{
	const int dp = ctx->schur.dp, dl = ctx->schur.dl;
	if(dp == 6 && dl == 3) schur_sparse_sigma_t<6, 3>(ctx, d_vals, d_sigma, inverse_only);
	else if(dp == 3 && dl == 2) schur_sparse_sigma_t<3, 2>(ctx, d_vals, d_sigma, inverse_only);
	else if(dp == 7 && dl == 3) schur_sparse_sigma_t<7, 3>(ctx, d_vals, d_sigma, inverse_only);
	else throw Error(SPP_E_UNSUPPORTED, "spp_schur_sparse_sigma_device: block widths not instantiated ({6,3}, {3,2}, {7,3})");
}

} // namespace spp
