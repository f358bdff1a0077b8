// spp_dense_trsm.h -- R^T R X = B for k right-hand sides against a factor that is already there (included by
// spp_dense.hip). R: upper, 128 x 128 tiles, leading dimension ld; T_J = R_JJ^-1 whole, in tinv_all.
//
// Right-looking, one step per block row (forward) / block column (backward):
//     forward  J = 0 .. nblk-1:  X_J = T_J^T B_J ;  B_I -= R_{J,I}^T X_J  for the tiles I > J
//     backward J = nblk-1 .. 0:  X_J = T_J   B_J ;  B_I -= R_{I,J}   X_J  for the tiles I < J
// The order of the steps comes from the stream alone: a launch per step (or two, SPP_TRSM_FUSED=0), nothing in here
// waits for another workgroup. Within a launch nobody writes what somebody else reads, because the finished blocks and
// the blocks still being updated live in two different panels:
//     forward : reads / updates B, stores the finished Y_J into the workspace W
//     backward: reads / updates W, stores the finished X_J into B
// so B is solved in place and W (nblk * 128 rows x 128 columns) is scratch.
//
// Every 16 x 16 tile of a product is one chain of v_mfma_f64_16x16x4_f64 over k ascending; a column of B meets the same
// operations whatever its neighbours are and wherever it stands, so column j of a k-column solve has the bits of that
// column solved alone. The matrix operand is read from memory as MFMA fragments (each element once per workgroup), the
// right-hand sides sit in LDS, k padded with zero columns to NCT * 16. Nothing of B outside rows [0, n) and its k columns
// is read or written; rows and columns of R from n on (identity padding, a right-hand side that rode along) are masked.
#pragma once

namespace spp {

constexpr int TRSM_THREADS = 512, TRSM_XS = NB + 2; // eight waves: a 16-row slab of the 128-row tile each; LDS column stride
// Matrix fragments (4 values of k each) a lane fetches at once. Up to 32 right-hand sides a lane holds ALL 32 fragments of
// its slab of T_J and all 32 of its slab of the target tile's R block, fetched at the very start together with B_J: a step
// is then one exposed memory round trip (measured on the Venice shape, k = 1: 24 us per step with the fetches in four
// dependent batches). Beyond that the accumulators need the registers: batches of 16.
template <int NCT> struct TrsmFrags { static constexpr int N = (NCT <= 2) ? NB / 4 : 16; };
// What a masked fragment reads instead (never written): an address select in front of the load, so no lane mask has to
// outlive the load (a value select behind it kept 32 masks alive and spilled scalar registers)
__device__ double trsm_zero_word;

// role 0: every workgroup forms X_J; workgroup 0 stores it, workgroup 1 + t updates target tile t  (one launch per step)
// role 1: the one workgroup forms X_J and stores it;  role 2: workgroup t loads the stored X_J and updates target tile t
template <bool FWD, int NCT>
__global__ __launch_bounds__(TRSM_THREADS)
void trsm_step_kernel(const double *__restrict__ R, int64_t ld, int64_t n, const double *__restrict__ tinv_all, int J, int role,
	double *cur, int64_t ldc, double *fin, int64_t ldf, int kc)
{
	extern __shared__ double trsm_xs[]; // X_J (before: B_J) as [column][row], NCT * 16 columns
	constexpr int KP = NCT * 16, FR = TrsmFrags<NCT>::N, NF = NB / 4, NST = KP * NB / TRSM_THREADS;
	constexpr bool EARLY = FR == NF;
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
	const int64_t J0 = (int64_t)J * NB;
	const int nv = (int)((n - J0 < NB) ? (n - J0) : NB);
	const bool solve = role != 2, update = role == 2 || (role == 0 && blockIdx.x > 0);
	const int i = wave * 16 + l15; // the row of the output tile this lane's matrix fragment belongs to
	const double *zero = &trsm_zero_word;
	// T_J (k, i) for X = T^T B, T_J (i, k) for X = T B: upper triangular, rows and columns from nv on masked
	const double *T = tinv_all + (size_t)J * NB * NB;
	auto t_addr = [&](const int k) {
		const bool in = FWD ? (k <= i && i < nv) : (i <= k && k < nv);
		return in ? (FWD ? T + k + (size_t)i * NB : T + i + (size_t)k * NB) : zero;
	};
	// forward: R_{J,I}(k, i), k the contiguous index; backward: R_{I,J}(i, k), i the contiguous index, columns from n on masked
	const int t = (int)blockIdx.x - (role == 0 ? 1 : 0);
	const int64_t I0 = (int64_t)(FWD ? J + 1 + t : t) * NB, row = I0 + i;
	const double *a_ptr = FWD ? R + J0 + row * ld : R + row + J0 * ld;
	const int64_t a_ks = FWD ? 1 : ld;
	auto r_addr = [&](const int k) { return (k < nv) ? a_ptr + k * a_ks : zero; };
	// T is upper triangular: row slab `wave` of T^T sees k < 16 (wave + 1), of T k >= 16 wave (wave-uniform bounds)
	const int kb = FWD ? 0 : wave * 16, ke = FWD ? (wave + 1) * 16 : NB, kend = (nv + 3) & ~3;
	v4f64 acc[NCT], old[NCT];
	double at[FR], ar[EARLY ? FR : 1];
	{
		// every fetch that does not depend on X_J is issued here, in front of the first barrier
		const double *src = solve ? cur : fin;
		const int64_t lds = solve ? ldc : ldf;
		if(EARLY) {
			double st[NST];
#pragma unroll
			for(int u = 0; u < NST; ++ u) {
				const int e = tid + u * TRSM_THREADS, r = e & (NB - 1), q = e >> 7;
				st[u] = *((r < nv && q < kc) ? src + J0 + r + (int64_t)q * lds : zero);
			}
			if(solve) {
#pragma unroll
				for(int j = 0; j < FR; ++ j)
					at[j] = *t_addr(4 * j + l4);
			}
			if(update) {
#pragma unroll
				for(int j = 0; j < FR; ++ j)
					ar[j] = *r_addr(4 * j + l4);
#pragma unroll
				for(int c = 0; c < NCT; ++ c)
#pragma unroll
					for(int r = 0; r < 4; ++ r) {
						const int q = c * 16 + l4 + 4 * r;
						old[c][r] = *((row < n && q < kc) ? cur + row + (int64_t)q * ldc : zero);
					}
			}
#pragma unroll
			for(int u = 0; u < NST; ++ u) {
				const int e = tid + u * TRSM_THREADS, r = e & (NB - 1), q = e >> 7;
				trsm_xs[q * TRSM_XS + r] = st[u];
			}
		} else {
#pragma unroll 4
			for(int u = 0; u < NST; ++ u) {
				const int e = tid + u * TRSM_THREADS, r = e & (NB - 1), q = e >> 7;
				trsm_xs[q * TRSM_XS + r] = *((r < nv && q < kc) ? src + J0 + r + (int64_t)q * lds : zero);
			}
		}
	}
	__syncthreads();
	if(solve) {
#pragma unroll
		for(int c = 0; c < NCT; ++ c)
			acc[c] = (v4f64){0, 0, 0, 0};
		if(EARLY) {
#pragma unroll
			for(int j = 0; j < FR; ++ j) {
				if(4 * j >= kb && 4 * j < ke) { // (wave-uniform)
#pragma unroll
					for(int c = 0; c < NCT; ++ c)
						acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(trsm_xs[(c * 16 + l15) * TRSM_XS + 4 * j + l4], at[j], acc[c], 0, 0, 0);
				}
			}
		} else {
#pragma unroll 1
			for(int h = 0; h < NF; h += FR) {
#pragma unroll
				for(int j = 0; j < FR; ++ j) {
					at[j] = 0.0;
					if(4 * (h + j) >= kb && 4 * (h + j) < ke)
						at[j] = *t_addr(4 * (h + j) + l4);
				}
#pragma unroll
				for(int j = 0; j < FR; ++ j) {
					if(4 * (h + j) >= kb && 4 * (h + j) < ke) {
#pragma unroll
						for(int c = 0; c < NCT; ++ c)
							acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(trsm_xs[(c * 16 + l15) * TRSM_XS + 4 * (h + j) + l4], at[j], acc[c], 0, 0, 0);
					}
				}
			}
		}
		__syncthreads(); // B_J has been read by every wave
#pragma unroll
		for(int c = 0; c < NCT; ++ c)
#pragma unroll
			for(int r = 0; r < 4; ++ r)
				trsm_xs[(c * 16 + l4 + 4 * r) * TRSM_XS + i] = acc[c][r];
		__syncthreads();
		if(!update) {
			for(int e = tid; e < KP * NB; e += TRSM_THREADS) {
				const int r = e & (NB - 1), q = e >> 7;
				if(r < nv && q < kc)
					fin[J0 + r + (int64_t)q * ldf] = trsm_xs[q * TRSM_XS + r];
			}
			return;
		}
	}
#pragma unroll
	for(int c = 0; c < NCT; ++ c)
		acc[c] = (v4f64){0, 0, 0, 0};
	if(EARLY) {
#pragma unroll
		for(int j = 0; j < FR; ++ j) {
			if(4 * j < kend) { // (workgroup-uniform)
#pragma unroll
				for(int c = 0; c < NCT; ++ c)
					acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(trsm_xs[(c * 16 + l15) * TRSM_XS + 4 * j + l4], ar[j], acc[c], 0, 0, 0);
			}
		}
	} else {
#pragma unroll 1
		for(int h = 0; h < NF; h += FR) {
#pragma unroll
			for(int j = 0; j < FR; ++ j) {
				at[j] = 0.0;
				if(4 * (h + j) < kend)
					at[j] = *r_addr(4 * (h + j) + l4);
			}
#pragma unroll
			for(int j = 0; j < FR; ++ j) {
				if(4 * (h + j) < kend) {
#pragma unroll
					for(int c = 0; c < NCT; ++ c)
						acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(trsm_xs[(c * 16 + l15) * TRSM_XS + 4 * (h + j) + l4], at[j], acc[c], 0, 0, 0);
				}
			}
		}
	}
#pragma unroll
	for(int c = 0; c < NCT; ++ c)
#pragma unroll
		for(int r = 0; r < 4; ++ r) {
			const int q = c * 16 + l4 + 4 * r;
			if(row < n && q < kc) // (the wide forms fetch the old value only here: their registers hold the accumulators)
				cur[row + (int64_t)q * ldc] = (EARLY ? old[c][r] : cur[row + (int64_t)q * ldc]) - acc[c][r];
		}
}

template <bool FWD, int NCT>
static void trsm_step_launch(hipStream_t s, int fused, int nblk, int J, const double *R, int64_t ld, int64_t n,
	const double *tinv_all, double *cur, int64_t ldc, double *fin, int64_t ldf, int kc)
{
	static uint64_t attr_seen = 0;
	const size_t lds = (size_t)NCT * 16 * TRSM_XS * sizeof(double);
	if(first_on_this_device(attr_seen))
		SPP_HIP_CHECK(hipFuncSetAttribute((const void*)trsm_step_kernel<FWD, NCT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
	const unsigned targets = (unsigned)(FWD ? nblk - 1 - J : J);
	if(fused)
		hipLaunchKernelGGL((trsm_step_kernel<FWD, NCT>), dim3(1 + targets), dim3(TRSM_THREADS), lds, s,
			R, ld, n, tinv_all, J, 0, cur, ldc, fin, ldf, kc);
	else {
		hipLaunchKernelGGL((trsm_step_kernel<FWD, NCT>), dim3(1), dim3(TRSM_THREADS), lds, s,
			R, ld, n, tinv_all, J, 1, cur, ldc, fin, ldf, kc);
		if(targets)
			hipLaunchKernelGGL((trsm_step_kernel<FWD, NCT>), dim3(targets), dim3(TRSM_THREADS), lds, s,
				R, ld, n, tinv_all, J, 2, cur, ldc, fin, ldf, kc);
	}
}

template <int NCT>
static void trsm_pass(spp_ctx *ctx, const double *R, int64_t n, int64_t ld, double *B, int64_t ldb, int kc)
{
	DenseWork &dw = ctx->dense;
	const int nblk = (int)((n + NB - 1) / NB), fused = switches().trsm_fused;
	const int64_t ldw = (int64_t)nblk * NB;
	double *W = dw.trsm_w.p;
	for(int J = 0; J < nblk; ++ J)
		trsm_step_launch<true, NCT>(ctx->stream, fused, nblk, J, R, ld, n, dw.tinv_all.p, B, ldb, W, ldw, kc);
	for(int J = nblk; J-- > 0;)
		trsm_step_launch<false, NCT>(ctx->stream, fused, nblk, J, R, ld, n, dw.tinv_all.p, W, ldw, B, ldb, kc);
}

// the stored block inverses become whole ones (what dense_potrs_upper does in front of its substitution)
void dense_tinv_complete(spp_ctx *ctx)
{
	if(ctx->dense.tinv_half > 0) {
		hipLaunchKernelGGL(tinv_finish_kernel, dim3((unsigned)ctx->dense.tinv_half), dim3(1024), 0, ctx->stream, ctx->dense.tinv_all.p);
		ctx->dense.tinv_half = 0;
	}
}

// R^T R X = B in place for the nrhs columns of B (n rows, leading dimension ldb), against the factor R (n x n, ld) and the
// block inverses the last factorization of this ctx left; at most 128 columns per pass
void dense_potrs_multi(spp_ctx *ctx, const double *d_R, int64_t n, int64_t ld, double *d_B, int64_t ldb, int64_t nrhs)
{
	SPP_REQUIRE(ld % NB == 0 && n > 0 && n < ld && ldb >= n && nrhs >= 1, SPP_E_BADARG, "dense_potrs_multi: bad extents");
	dense_tinv_complete(ctx);
	const int64_t nblk = (n + NB - 1) / NB;
	ctx->dense.trsm_w.reserve((size_t)nblk * NB * NB);
	for(int64_t c0 = 0; c0 < nrhs; c0 += NB) {
		const int kc = (int)std::min<int64_t>(NB, nrhs - c0);
		double *B = d_B + c0 * ldb;
		if(kc <= 16) trsm_pass<1>(ctx, d_R, n, ld, B, ldb, kc);
		else if(kc <= 32) trsm_pass<2>(ctx, d_R, n, ld, B, ldb, kc);
		else if(kc <= 64) trsm_pass<4>(ctx, d_R, n, ld, B, ldb, kc);
		else trsm_pass<8>(ctx, d_R, n, ld, B, ldb, kc);
	}
	SPP_HIP_CHECK(hipGetLastError());
}

} // namespace spp
