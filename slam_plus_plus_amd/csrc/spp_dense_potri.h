// spp_dense_potri.h -- Z = (R^T R)^-1, the full symmetric inverse, from a factor that is already there (included by
// spp_dense.hip behind spp_dense_trsm.h). R: upper, 128 x 128 tiles, leading dimension ld; T_J = R_JJ^-1 whole, in tinv_all.
//
// Block rows J descending (R Z = R^-T, whose blocks above the diagonal are zero and whose diagonal blocks are T_J^T):
//     Z[J, K] = T_J (delta_JK T_J^T - sum_{I > J} R[J, I] Z[I, K])      for the tiles K >= J
// and Z[I, J], I > J, is the mirror of the row just formed: both triangles are stored, so every operand is a plain block.
// The diagonal tile needs Z[I, J] = Z[J, I]^T of its own row, hence three launches per block row, in stream order:
//     1  potri_row_kernel<false>   Z[J, K], K > J     reads rows I > J of Z (all finished), writes row J right of the diagonal
//     2  potri_mirror_kernel       Z[K, J] = Z[J, K]^T  reads what 1 wrote, writes column J below the diagonal
//     3  potri_row_kernel<true>    Z[J, J]            reads what 2 wrote, writes the diagonal tile: its upper triangle and
//                                                      the mirror of it, so Z is exactly symmetric
// Order comes from the stream alone, nothing in here waits for another workgroup, and within a launch nobody writes what
// somebody else reads. A workgroup owns block row J and 16 columns; wave w owns the 16-row slab w. Every 16 x 16 tile of a
// product is one chain of v_mfma_f64_16x16x4_f64, I ascending and k ascending inside a block: the order is fixed by the
// shape alone. The slab of R comes from memory as MFMA fragments (each element once per workgroup), the rows of Z through
// LDS. Rows and columns from n on -- of R, T and Z -- are masked by the address select of trsm_step_kernel: nothing of Z
// outside [0, n) x [0, n) is read or written, R and tinv_all are only read, the tile mask is not used (unlisted tiles of R
// are zero).
#pragma once

namespace spp {

constexpr int POTRI_THREADS = 512, POTRI_XS = NB + 2, POTRI_NC = 16; // eight waves; LDS column stride; columns per workgroup

template <bool DIAG>
__global__ __launch_bounds__(POTRI_THREADS)
void potri_row_kernel(const double *__restrict__ R, int64_t ld, int64_t n, const double *__restrict__ tinv_all, int J, int nblk,
	double *Z, int64_t ldz)
{
	__shared__ double xs[POTRI_NC * POTRI_XS]; // a 128 x 16 block of Z, then of the right-hand side, as [column][row]
	constexpr int NF = NB / 4, NST = POTRI_NC * NB / POTRI_THREADS;
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
	const int64_t J0 = (int64_t)J * NB;
	const int nv = (int)((n - J0 < NB) ? (n - J0) : NB);
	const int i = wave * 16 + l15; // the row of block row J this lane's matrix fragments belong to
	const int64_t c0 = (DIAG ? J0 : J0 + NB) + (int64_t)blockIdx.x * POTRI_NC; // first column of this workgroup
	const double *zero = &trsm_zero_word;
	const double *T = tinv_all + (size_t)J * NB * NB;
	const double *r_row = R + J0 + i;
	auto r_addr = [&](const int64_t I0, const int k) { return (i < nv && I0 + k < n) ? r_row + (I0 + k) * ld : zero; };
	auto z_addr = [&](const int64_t I0, const int u) {
		const int e = tid + u * POTRI_THREADS, r = e & (NB - 1), q = e >> 7;
		return (I0 + r < n && c0 + q < n) ? (const double*)Z + I0 + r + (c0 + q) * ldz : zero;
	};
	v4f64 acc = (v4f64){0, 0, 0, 0};
	double ar[NF], st[NST];
	// (a block behind the last one reads the zero word throughout: the fetches need no branch)
#pragma unroll
	for(int u = 0; u < NST; ++ u)
		st[u] = *z_addr(J0 + NB, u);
#pragma unroll
	for(int j = 0; j < NF; ++ j)
		ar[j] = *r_addr(J0 + NB, 4 * j + l4);
#pragma unroll 1
	for(int I = J + 1; I < nblk; ++ I) {
		const int64_t I1 = (int64_t)(I + 1) * NB;
		__syncthreads(); // the block before this one has been read by every wave
#pragma unroll
		for(int u = 0; u < NST; ++ u) {
			const int e = tid + u * POTRI_THREADS;
			xs[(e >> 7) * POTRI_XS + (e & (NB - 1))] = st[u];
		}
		__syncthreads();
		// the next block's fetches fly while this one's products run: every register is refilled as soon as it was used
#pragma unroll
		for(int u = 0; u < NST; ++ u)
			st[u] = *z_addr(I1, u);
#pragma unroll
		for(int j = 0; j < NF; ++ j) {
			acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xs[l15 * POTRI_XS + 4 * j + l4], ar[j], acc, 0, 0, 0);
			ar[j] = *r_addr(I1, 4 * j + l4);
		}
	}
	__syncthreads();
	// the right-hand side of the block row: delta_JK T_J^T - sum; lane holds row i, columns l4 + 4 r
#pragma unroll
	for(int r = 0; r < 4; ++ r) {
		const int q = l4 + 4 * r;
		double d = 0;
		if(DIAG) {
			const int cl = (int)blockIdx.x * POTRI_NC + q; // T_J^T (i, cl) = T_J (cl, i)
			d = *((cl <= i && i < nv) ? T + cl + (size_t)i * NB : zero);
		}
		xs[q * POTRI_XS + i] = d - acc[r];
	}
	// T_J (i, k): upper triangular, rows and columns from nv on masked; row slab `wave` sees k >= 16 wave. Fetched here, not
	// in front of the loop: with the loop's fragments and their addresses they would not fit the registers of 512 threads
#pragma unroll
	for(int j = 0; j < NF; ++ j) {
		const int k = 4 * j + l4;
		ar[j] = *((i <= k && k < nv) ? T + i + (size_t)k * NB : zero);
	}
	__syncthreads();
	acc = (v4f64){0, 0, 0, 0};
#pragma unroll
	for(int j = 0; j < NF; ++ j) {
		if(4 * j >= wave * 16) // (wave-uniform)
			acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xs[l15 * POTRI_XS + 4 * j + l4], ar[j], acc, 0, 0, 0);
	}
	const int64_t row = J0 + i;
#pragma unroll
	for(int r = 0; r < 4; ++ r) {
		const int64_t col = c0 + l4 + 4 * r;
		if(i < nv && col < n) {
			if(!DIAG)
				Z[row + col * ldz] = acc[r];
			else if(col >= row) { // the upper triangle of the diagonal tile, and its mirror
				Z[row + col * ldz] = acc[r];
				if(col > row)
					Z[col + row * ldz] = acc[r];
			}
		}
	}
}

// Z[c, r] = Z[r, c] for the rows r of block row J and the columns c right of its diagonal tile
__global__ __launch_bounds__(256)
void potri_mirror_kernel(int J, int64_t n, double *Z, int64_t ldz)
{
	__shared__ double t[32][33];
	const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
	const int64_t J0 = (int64_t)J * NB, rend = (n - J0 < NB) ? n : J0 + NB;
	const int64_t r0 = J0 + (int64_t)blockIdx.y * 32, c0 = J0 + NB + (int64_t)blockIdx.x * 32;
#pragma unroll
	for(int s = 0; s < 4; ++ s) {
		const int64_t r = r0 + tx, c = c0 + ty + 8 * s;
		t[ty + 8 * s][tx] = (r < rend && c < n) ? Z[r + c * ldz] : 0.0;
	}
	__syncthreads();
#pragma unroll
	for(int s = 0; s < 4; ++ s) {
		const int64_t r = r0 + ty + 8 * s, c = c0 + tx;
		if(r < rend && c < n)
			Z[c + r * ldz] = t[tx][ty + 8 * s];
	}
}

// Z (n x n, leading dimension ldz, both triangles) <- (R^T R)^-1 against the factor R (n x n, ld) and the block inverses
// the last factorization of this ctx left; three launches per block row on the ctx stream, nothing else
void dense_potri_upper(spp_ctx *ctx, const double *d_R, int64_t n, int64_t ld, double *d_Z, int64_t ldz)
{
	SPP_REQUIRE(ld % NB == 0 && n > 0 && n < ld && ldz >= n, SPP_E_BADARG, "dense_potri_upper: bad extents");
	dense_tinv_complete(ctx);
	hipStream_t s = ctx->stream;
	const double *tinv_all = ctx->dense.tinv_all.p;
	const int nblk = (int)((n + NB - 1) / NB);
	for(int J = nblk; J-- > 0;) {
		const int64_t J0 = (int64_t)J * NB, nv = std::min<int64_t>(NB, n - J0), right = n - J0 - nv;
		if(right > 0) {
			hipLaunchKernelGGL((potri_row_kernel<false>), dim3((unsigned)((right + POTRI_NC - 1) / POTRI_NC)), dim3(POTRI_THREADS), 0, s,
				d_R, ld, n, tinv_all, J, nblk, d_Z, ldz);
			hipLaunchKernelGGL(potri_mirror_kernel, dim3((unsigned)((right + 31) / 32), (unsigned)((nv + 31) / 32)), dim3(256), 0, s,
				J, n, d_Z, ldz);
		}
		hipLaunchKernelGGL((potri_row_kernel<true>), dim3((unsigned)((nv + POTRI_NC - 1) / POTRI_NC)), dim3(POTRI_THREADS), 0, s,
			d_R, ld, n, tinv_all, J, nblk, d_Z, ldz);
	}
	SPP_HIP_CHECK(hipGetLastError());
}

} // namespace spp
