// spp_sparse_sigma.hip -- the blocks of Sigma = Lambda^-1 on the stored pattern of Lambda, by selected inversion on the
// multifrontal factor a sparse solve left behind.
//
// Front s keeps its w pivot rows of R: R11 (w x w, upper) and R12 (w x m, m = h - 1 - w), R[i, c] = F[i + padded(c, w, pad) * ld].
// Z_s is Sigma on the front's h - 1 indices, kept in a second arena (`sigma_z`) at the fronts' own offsets, leading
// dimensions and padding, both triangles stored. Down the assembly tree, levels descending, per front
//     1  Z22[a, b] = Z_parent[rel[a], rel[b]]                       (a root has m = 0)
//     2  Z12 = -R11^-1 (R12 Z22), Z21 its transpose                 one backward substitution per column of Z22
//     3  Z11 = R11^-1 (R11^-T - R12 Z21)                            per pivot column c: y = R11^-T e_c forward, then backward;
//                                                                   rows <= c are kept and mirrored: exactly symmetric
// and at the end one gather runs the assembly map backwards: every stored block of Lambda has one entry in asm_src /
// asm_dst / asm_shape, so every double of d_sigma is written once.
// Steps 2 and 3 are substitutions with m and w independent columns; a workgroup owns (front, 16 columns of Z) and the
// column tiles of a front spread over the grid. Per level: steps 1 + 2 in one launch (a workgroup fetches the columns of
// Z22 it owns; classes 3 - 4: step 1 is a launch of its own, sg_fetch_kernel), step 3 in the next, each once for the
// fronts of classes 0 - 2 and once for those of classes 3 - 4 -- the body is chosen by the front's size class alone.
//   classes 0 - 2  sg_cols_kernel: the pivot rows of R and the 16 work columns in LDS, every entry one chain of explicit
//                  fused multiply-adds in a fixed order (the bodies of ss_fwd_kernel / ss_bwd_kernel, spp_sparse_solve.hip);
//   classes 3 - 4  sg_cols_mfma_kernel: sixteen waves, the work columns are the columns of Z themselves, the products are
//                  chains of v_mfma_f64_16x16x4_f64 split over the waves by the front's shape alone and summed in wave
//                  order (the bodies of ss_fwd_mfma_kernel / ss_bwd_mfma_kernel); Z21 and the lower triangle of Z11 are
//                  mirrored by launches of their own (sg_mirror_kernel): a column under work is nobody else's to write.
// The parent is finished by the launch boundary; inside a launch a workgroup reads R, its parent's Z and its own columns
// of Z and writes its own columns (classes 0 - 2: also their mirror rows, which nobody reads before the next launch). No
// flags, no waits. A column of Z meets the same instruction sequence wherever it lands in a tile.

#include "spp_internal.h"
#include "spp_sparse_plan.h"
#include "spp_tiles.h"
#include <algorithm>

namespace spp {

constexpr int SG_NT = 256;          // threads of a workgroup of the LDS body
constexpr int SG_CW = 16;           // columns of Z a workgroup owns
constexpr int SG_PB = 16;           // pivots of a block of the triangular solves
constexpr int SG_MT = 1024;         // threads of a workgroup of the MFMA body
constexpr int SG_MW = SG_MT / 64;   // its waves
// the largest front of class 2 (w = 112, h - 1 = 127): its pivot rows at column stride w | 1 beside 16 work columns
constexpr size_t SG_LDS_MAX = (size_t)(113 * 127 + 127 * SG_CW) * sizeof(double);

__device__ const double sg_zero_word = 0.0;

// the 16 x 16 diagonal tile at pivot j0 into LDS (R[i, k] at tri[i + k * 17], upper triangle); beyond the nb valid pivots
// the identity. Masked by address select in front of the load: every lane loads, none outside the front.
__device__ __forceinline__ void sg_stage_tri(const double *F, int ld, int j0, int nb, double *tri)
{
	if(threadIdx.x < SG_PB * SG_PB) {
		const int e = threadIdx.x, i = e & 15, k = e >> 4;
		const bool in = i <= k && k < nb;
		const double v = *(in ? F + (j0 + i) + (int64_t)(j0 + k) * ld : F);
		tri[i + k * 17] = in ? v : (i == k ? 1.0 : 0.0);
	}
}

// forward sweep of the staged tile over the 16 entries of one column held by 16 lanes (R^T y = t)
__device__ __forceinline__ double sg_sweep_fwd(double t, const double *tri, int r, int lane)
{
#pragma unroll
	for(int i = 0; i < SG_PB; ++ i) {
		const double yi = __shfl(t, (lane & 48) + i) / tri[i + i * 17];
		t = (r == i) ? yi : ((r > i) ? __builtin_fma(-tri[i + r * 17], yi, t) : t);
	}
	return t;
}

// backward sweep (R x = t), from the last pivot up
__device__ __forceinline__ double sg_sweep_bwd(double t, const double *tri, int r, int lane)
{
#pragma unroll
	for(int i = SG_PB - 1; i >= 0; -- i) {
		const double xi = __shfl(t, (lane & 48) + i) / tri[i + i * 17];
		t = (r == i) ? xi : ((r < i) ? __builtin_fma(-tri[r + i * 17], xi, t) : t);
	}
	return t;
}

// ---- classes 0 - 2 ---------------------------------------------------------------------------------------------------
// PIV = false: the columns w .. h - 2 of Z (steps 1 and 2), PIV = true: the pivot columns (step 3). Dynamic LDS:
// ((w | 1) (h - 1) + 16 (h - 1)) doubles, a launch asks for its largest front's.
template <bool PIV>
__global__ __launch_bounds__(SG_NT)
void sg_cols_kernel(const SigmaFront *__restrict__ desc, const double *__restrict__ fronts, double *zs, const int32_t *__restrict__ rel)
{
	constexpr int CW = SG_CW, NR = SG_NT / CW;
	extern __shared__ double sg_sm[];
	__shared__ double tri[SG_PB * 17];
	__shared__ double ts[SG_PB * CW];
	const SigmaFront fd = desc[blockIdx.x];
	const int h = fd.h, w = fd.w, ld = fd.ld, pad = fd.pad;
	const int hc = h - 1, ws = w | 1, m = hc - w;
	const int ncols = PIV ? w : m;
	const int c0 = (int)blockIdx.y * CW;
	if(c0 >= ncols)
		return; // (the grid is as wide as the level's widest front)
	double *Rs = sg_sm, *T = sg_sm + ws * hc; // R[i, c] at Rs[i + c * ws]; entry r of column col at T[r * CW + col]
	const double *F = fronts + fd.off;
	double *Z = zs + fd.off;
	const int tid = threadIdx.x, lane = tid & 63, col = tid % CW, q = tid / CW;
	for(int e = tid; e < w * hc; e += SG_NT) {
		const int i = e % w, c = e / w;
		Rs[i + c * ws] = F[i + (int64_t)padded(c, w, pad) * ld];
	}
	// the work columns: e_c over Z21[:, c] (PIV), 0 over Z22[:, c] fetched from the parent and kept (otherwise); a column
	// beyond the front's last is solved on zeros and never stored
	for(int e = tid; e < hc * CW; e += SG_NT) {
		const int r = e % hc, cl = e / hc, c = c0 + cl;
		double v = 0.0;
		if(c < ncols) {
			if(PIV)
				v = r < w ? (r == c ? 1.0 : 0.0) : Z[(r + pad) + (int64_t)c * ld];
			else if(r >= w) {
				const int32_t *rl = rel + fd.relp;
				v = zs[fd.poff + padded(rl[r - w], fd.pw, fd.ppad) + (int64_t)padded(rl[c], fd.pw, fd.ppad) * fd.pld];
				Z[(r + pad) + (int64_t)(w + pad + c) * ld] = v;
			}
		}
		T[r * CW + cl] = v;
	}
	__syncthreads();
	if(PIV) {
		// ---- y = R11^-T e_c, 16 pivots per block from the tile's first column on (the rows above it stay zero): the
		// products with the blocks above, then the diagonal tile
		for(int j0 = c0; j0 < w; j0 += SG_PB) {
			const int nb = (w - j0 < SG_PB) ? w - j0 : SG_PB;
			sg_stage_tri(Rs, ws, j0, nb, tri);
			if(q < SG_PB) {
				double acc = 0.0;
				if(q < nb) {
					const double *Rc = Rs + (j0 + q) * ws;
					acc = T[(j0 + q) * CW + col];
					for(int p = c0; p < j0; ++ p)
						acc = __builtin_fma(-Rc[p], T[p * CW + col], acc);
				}
				ts[q * CW + col] = acc;
			}
			__syncthreads();
			{ // lane group of 16 = the 16 entries of one column
				const int r = tid & 15, cc = tid >> 4;
				const double t = sg_sweep_fwd(ts[r * CW + cc], tri, r, lane);
				if(r < nb)
					T[(j0 + r) * CW + cc] = t;
			}
			__syncthreads();
		}
	}
	// ---- x = R11^-1 (y - R12 t), 16 pivots per block from the last one up: everything right of the block, then the tile
	for(int j0 = ((w - 1) / SG_PB) * SG_PB; j0 >= 0; j0 -= SG_PB) {
		const int nb = (w - j0 < SG_PB) ? w - j0 : SG_PB;
		sg_stage_tri(Rs, ws, j0, nb, tri);
		if(q < SG_PB) {
			double acc = 0.0;
			if(q < nb) {
				const double *Rr = Rs + j0 + q;
				acc = T[(j0 + q) * CW + col];
				for(int c = j0 + nb; c < hc; ++ c)
					acc = __builtin_fma(-Rr[c * ws], T[c * CW + col], acc);
			}
			ts[q * CW + col] = acc;
		}
		__syncthreads();
		{
			const int r = tid & 15, cc = tid >> 4;
			const double t = sg_sweep_bwd(ts[r * CW + cc], tri, r, lane);
			if(r < nb)
				T[(j0 + r) * CW + cc] = t;
		}
		__syncthreads();
	}
	// the column and its mirror row; of a pivot column the rows up to the diagonal
	for(int e = tid; e < w * CW; e += SG_NT) {
		const int r = e % w, cl = e / w, c = c0 + cl;
		if(c < ncols && (!PIV || r <= c)) {
			const double v = T[r * CW + cl];
			const int cc = PIV ? c : w + pad + c;
			Z[r + (int64_t)cc * ld] = v;
			Z[cc + (int64_t)r * ld] = v;
		}
	}
}

// ---- classes 3 - 4 ---------------------------------------------------------------------------------------------------
// D[i][j] += sum over 16 inner indices of A[k][i] B[k][j]; the lane holds A[4 kk + l4][l15], B[4 kk + l4][l15] and
// D[l4 + 4 r][l15] (the layout of tile_atb, spp_tiles.h)
__device__ __forceinline__ v4f64 sg_mfma16(const double *const pa[4], const double *const pb[4], v4f64 acc)
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

// The work columns are the tile's own columns of Z in the arena (row stride 1, column stride ld): step 2 finds Z22 in
// their rows w .. h - 2 (sg_fetch_kernel, the launch before) and clears the pivot rows, step 3 finds Z21 there and sets
// e_c. The products in front of a 16-pivot block are split over the waves by 16-blocks of the inner index, each wave ONE
// chain of MFMAs over its blocks ascending, the partial tiles summed in wave order. Operands are masked by an address
// select in front of the load (a masked lane reads sg_zero_word): rows and columns beyond the front's are never touched.
template <bool PIV>
__global__ __launch_bounds__(SG_MT)
void sg_cols_mfma_kernel(const SigmaFront *__restrict__ desc, const double *__restrict__ fronts, double *zs)
{
	constexpr int CW = SG_CW;
	__shared__ double tri[SG_PB * 17];
	__shared__ double ts[SG_PB * CW];
	__shared__ double part[SG_MW][SG_PB * CW];
	const SigmaFront fd = desc[blockIdx.x];
	const int h = fd.h, w = fd.w, ld = fd.ld, pad = fd.pad;
	const int hc = h - 1, m = hc - w;
	const int ncols = PIV ? w : m;
	const int c0 = (int)blockIdx.y * CW;
	if(c0 >= ncols)
		return;
	const double *F = fronts + fd.off;
	double *Z = zs + fd.off;
	const int tid = threadIdx.x, col = tid % CW, q = tid / CW;
	const int lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
	// a tile column beyond the front's last works on a copy of the last one and is never stored: no mask to carry
	const int last = ncols - 1 - c0;
	const int cbase = PIV ? c0 : w + pad + c0;     // first column of the tile in the padded image
	const double *Zc = Z + (int64_t)(cbase + (col < last ? col : last)) * ld; // column `col` of the tile
	const double *Zb = Z + (int64_t)(cbase + (l15 < last ? l15 : last)) * ld; // B operand: entry p of column l15 of the tile
	// (sixteen waves, sixteen columns: wave v fills column v of the tile)
	if(c0 + wave < ncols) {
		double *Zw = Z + (int64_t)(cbase + wave) * ld;
		if(PIV) {
			for(int r = lane; r < w; r += 64)
				Zw[r] = (r == c0 + wave) ? 1.0 : 0.0;
		} else {
			for(int r = lane; r < w; r += 64)
				Zw[r] = 0.0;
		}
	}
	__syncthreads();
	if(PIV) {
		// ---- y = R11^-T e_c from the tile's first column on
		for(int j0 = c0; j0 < w; j0 += SG_PB) {
			const int nb = (w - j0 < SG_PB) ? w - j0 : SG_PB;
			sg_stage_tri(F, ld, j0, nb, tri);
			{
				v4f64 acc = (v4f64){0, 0, 0, 0};
				const bool ci = l15 < nb; // column j0 + l15 of R is a pivot column
				for(int p0 = c0 + wave * SG_PB; p0 < j0; p0 += SG_MW * SG_PB) { // (p0 + 15 < j0 <= w: rows in range)
					const double *pa[4], *pb[4];
#pragma unroll
					for(int kk = 0; kk < 4; ++ kk) {
						const int p = p0 + 4 * kk + l4;
						pa[kk] = ci ? F + p + (int64_t)(j0 + l15) * ld : &sg_zero_word;
						pb[kk] = Zb + p;
					}
					acc = sg_mfma16(pa, pb, acc);
				}
#pragma unroll
				for(int r = 0; r < 4; ++ r)
					part[wave][(l4 + 4 * r) * CW + l15] = acc[r];
			}
			__syncthreads();
			if(q < SG_PB) {
				double t = q < nb ? Zc[j0 + q] : 0.0;
#pragma unroll
				for(int v = 0; v < SG_MW; ++ v)
					t -= part[v][q * CW + col];
				ts[q * CW + col] = q < nb ? t : 0.0;
			}
			__syncthreads();
			if(tid < SG_PB * CW) { // waves 0 - 3: lane group of 16 = the 16 entries of one column
				const int r = tid & 15, cc = tid >> 4;
				const double t = sg_sweep_fwd(ts[r * CW + cc], tri, r, lane);
				if(r < nb && c0 + cc < ncols)
					Z[(j0 + r) + (int64_t)(cbase + cc) * ld] = t;
			}
			__syncthreads();
		}
	}
	// ---- x = R11^-1 (y - R12 t)
	for(int j0 = ((w - 1) / SG_PB) * SG_PB; j0 >= 0; j0 -= SG_PB) {
		const int nb = (w - j0 < SG_PB) ? w - j0 : SG_PB;
		sg_stage_tri(F, ld, j0, nb, tri);
		{
			v4f64 acc = (v4f64){0, 0, 0, 0};
			const bool ri = l15 < nb; // row j0 + l15 of R is a pivot row
			const double *Fr = F + j0 + l15;
			// the 16-blocks right of the block: n1 inside the pivot columns (from j0 + 16), then n2 beyond (from w)
			const int n1 = (w - (j0 + nb) + SG_PB - 1) / SG_PB, n2 = (m + SG_PB - 1) / SG_PB;
			for(int b = wave; b < n1 + n2; b += SG_MW) {
				const double *pa[4], *pb[4];
				if(b < n1) {
#pragma unroll
					for(int kk = 0; kk < 4; ++ kk) {
						const int c = j0 + nb + b * SG_PB + 4 * kk + l4;
						pa[kk] = (ri && c < w) ? Fr + (int64_t)c * ld : &sg_zero_word;
						pb[kk] = c < w ? Zb + c : &sg_zero_word;
					}
				} else {
#pragma unroll
					for(int kk = 0; kk < 4; ++ kk) {
						const int c = w + (b - n1) * SG_PB + 4 * kk + l4;
						const bool in = c < hc;
						pa[kk] = (ri && in) ? Fr + (int64_t)(c + pad) * ld : &sg_zero_word;
						pb[kk] = in ? Zb + c + pad : &sg_zero_word;
					}
				}
				acc = sg_mfma16(pa, pb, acc);
			}
#pragma unroll
			for(int r = 0; r < 4; ++ r)
				part[wave][(l4 + 4 * r) * CW + l15] = acc[r];
		}
		__syncthreads();
		if(q < SG_PB) {
			double t = q < nb ? Zc[j0 + q] : 0.0;
#pragma unroll
			for(int v = 0; v < SG_MW; ++ v)
				t -= part[v][q * CW + col];
			ts[q * CW + col] = q < nb ? t : 0.0;
		}
		__syncthreads();
		if(tid < SG_PB * CW) {
			const int r = tid & 15, cc = tid >> 4;
			const double t = sg_sweep_bwd(ts[r * CW + cc], tri, r, lane);
			if(r < nb && c0 + cc < ncols)
				Z[(j0 + r) + (int64_t)(cbase + cc) * ld] = t;
		}
		__syncthreads();
	}
}

// step 1 of the fronts of classes 3 - 4: Z22 from the parent, a workgroup per (front, 16 columns), a wave per column
__global__ __launch_bounds__(SG_NT)
void sg_fetch_kernel(const SigmaFront *__restrict__ desc, double *zs, const int32_t *__restrict__ rel)
{
	const SigmaFront fd = desc[blockIdx.x];
	const int w = fd.w, pad = fd.pad, m = fd.h - 1 - w;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int32_t *rl = rel + fd.relp;
	for(int c = (int)blockIdx.y * SG_CW + wave; c < m && c < ((int)blockIdx.y + 1) * SG_CW; c += SG_NT / 64) {
		double *Zw = zs + fd.off + (w + pad) + (int64_t)(w + pad + c) * fd.ld;
		const double *Zp = zs + fd.poff + (int64_t)padded(rl[c], fd.pw, fd.ppad) * fd.pld;
		for(int r = lane; r < m; r += 64)
			Zw[r] = Zp[padded(rl[r], fd.pw, fd.ppad)];
	}
}

// the mirror images the fronts of classes 3 - 4 still lack, a workgroup per (front, 16 columns), a wave per column:
// UPD: Z21 from Z12 behind step 2 (read by step 3 and by the children), otherwise the lower triangle of Z11 behind step 3.
// A launch of its own: a column under work in sg_cols_mfma_kernel is nobody else's to write.
template <bool UPD>
__global__ __launch_bounds__(SG_NT)
void sg_mirror_kernel(const SigmaFront *__restrict__ desc, double *zs)
{
	const SigmaFront fd = desc[blockIdx.x];
	const int w = fd.w, ld = fd.ld, ncols = UPD ? fd.h - 1 - w : w;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	double *Z = zs + fd.off;
	for(int c = (int)blockIdx.y * SG_CW + wave; c < ncols && c < ((int)blockIdx.y + 1) * SG_CW; c += SG_NT / 64) {
		const int cc = UPD ? w + fd.pad + c : c;
		for(int r = UPD ? lane : c + 1 + lane; r < w; r += 64)
			Z[UPD ? cc + (int64_t)r * ld : r + (int64_t)cc * ld] = Z[UPD ? r + (int64_t)cc * ld : cc + (int64_t)r * ld];
	}
}

// the assembly map backwards: a workgroup per front, a wave per stored block of Lambda, a lane per double
__global__ __launch_bounds__(SG_NT)
void sg_gather_kernel(const int64_t *__restrict__ front_off, const int32_t *__restrict__ front_w, const int32_t *__restrict__ front_ld,
	const int32_t *__restrict__ front_pad, const int32_t *__restrict__ asm_ptr, const int64_t *__restrict__ asm_src,
	const int32_t *__restrict__ asm_dst, const int32_t *__restrict__ asm_shape, const double *__restrict__ zs, double *__restrict__ sigma)
{
	const int s = blockIdx.x;
	const int w = front_w[s], ld = front_ld[s], pad = front_pad[s];
	const double *Z = zs + front_off[s];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	for(int q = asm_ptr[s] + wave; q < asm_ptr[s + 1]; q += SG_NT / 64) {
		const int64_t so = asm_src[q];
		double *dst = sigma + (so >> 1);
		const int dr = padded(asm_dst[q] & 0xffff, w, pad), dc = padded(asm_dst[q] >> 16, w, pad);
		const int nr = asm_shape[q] & 0xff, ncol = asm_shape[q] >> 8;
		if(lane < nr * ncol) {
			const int r = lane % nr, c = lane / nr;
			dst[(so & 1) ? c + ncol * r : r + nr * c] = Z[(dr + r) + (int64_t)(dc + c) * ld];
		}
	}
}

void sparse_sigma(spp_ctx *ctx, double *d_sigma)
{
	SparsePlan *sp = ctx->sparse;
	SPP_REQUIRE(sp, SPP_E_STATE, "sparse plan missing");
	hipStream_t s = ctx->stream;
	const int64_t ns = sp->n_snodes;
	if(sp->h_sigma_desc.empty()) { // (the host image lives in the plan: its upload may still run when this call returns)
		sp->h_sigma_desc.resize((size_t)ns);
		std::vector<int32_t> relp((size_t)ns + 1, 0); // rel_ptr, rebuilt: one entry per update row and the slot, roots none
		for(int64_t f = 0; f < ns; ++ f)
			relp[f + 1] = relp[f] + (sp->h_front_parent[f] >= 0 ? sp->h_front_h[f] - sp->h_front_w[f] : 0);
		sp->h_sigma_level.assign((size_t)sp->n_levels * 5, 0);
		for(int64_t l = 0; l < sp->n_levels; ++ l)
			for(int32_t i = sp->h_cls_ptr[l * NCLS]; i < sp->h_cls_ptr[l * NCLS + 5]; ++ i) {
				const int32_t f = sp->h_level_fronts[i], p = sp->h_front_parent[f];
				SigmaFront &d = sp->h_sigma_desc[i];
				d.off = sp->h_front_off[f];
				d.h = sp->h_front_h[f]; d.w = sp->h_front_w[f]; d.ld = sp->h_front_ld[f]; d.pad = sp->h_front_pad[f];
				d.poff = p >= 0 ? sp->h_front_off[p] : 0;
				d.pw = p >= 0 ? sp->h_front_w[p] : 0; d.ppad = p >= 0 ? sp->h_front_pad[p] : 0; d.pld = p >= 0 ? sp->h_front_ld[p] : 0;
				d.relp = relp[f];
				SPP_REQUIRE(p >= 0 || d.h - 1 == d.w, SPP_E_HIP, "internal: a root front with update rows");
				// per level: dynamic LDS of the class 0 - 2 launches, tiles of 16 update / pivot columns of either body
				int32_t *lv = sp->h_sigma_level.data() + l * 5;
				const int32_t hc = d.h - 1, tu = (hc - d.w + SG_CW - 1) / SG_CW, tp = (d.w + SG_CW - 1) / SG_CW;
				if(i < sp->h_cls_ptr[l * NCLS + 3]) {
					lv[0] = std::max(lv[0], ((d.w | 1) + SG_CW) * hc);
					lv[1] = std::max(lv[1], tu); lv[2] = std::max(lv[2], tp);
				} else {
					lv[3] = std::max(lv[3], tu); lv[4] = std::max(lv[4], tp);
				}
			}
		sp->sigma_desc.upload(sp->h_sigma_desc, s);
		sp->sigma_z.reserve((size_t)std::max<int64_t>(sp->front_doubles, 2));
	}
	static uint64_t attr_seen = 0;
	if(first_on_this_device(attr_seen)) {
		SPP_HIP_CHECK(hipFuncSetAttribute((const void*)sg_cols_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SG_LDS_MAX));
		SPP_HIP_CHECK(hipFuncSetAttribute((const void*)sg_cols_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SG_LDS_MAX));
	}
	const double *F = sp->fronts.p;
	double *Z = sp->sigma_z.p;
	const int32_t *rel = sp->rel.p;
	for(int64_t l = sp->n_levels; l > 0;) {
		-- l;
		const int32_t *cp = sp->h_cls_ptr.data() + l * NCLS, *lv = sp->h_sigma_level.data() + l * 5;
		const unsigned n_lo = (unsigned)(cp[3] - cp[0]), n_hi = (unsigned)(cp[5] - cp[3]);
		const SigmaFront *d_lo = sp->sigma_desc.p + cp[0], *d_hi = sp->sigma_desc.p + cp[3];
		const size_t lds = (size_t)lv[0] * sizeof(double);
		SPP_REQUIRE(lds <= SG_LDS_MAX, SPP_E_HIP, "internal: a front of classes 0 - 2 beyond the LDS of its body");
		if(n_lo && lv[1])
			hipLaunchKernelGGL(sg_cols_kernel<false>, dim3(n_lo, (unsigned)lv[1]), dim3(SG_NT), lds, s, d_lo, F, Z, rel);
		if(n_hi && lv[3]) {
			hipLaunchKernelGGL(sg_fetch_kernel, dim3(n_hi, (unsigned)lv[3]), dim3(SG_NT), 0, s, d_hi, Z, rel);
			hipLaunchKernelGGL(sg_cols_mfma_kernel<false>, dim3(n_hi, (unsigned)lv[3]), dim3(SG_MT), 0, s, d_hi, F, Z);
			hipLaunchKernelGGL(sg_mirror_kernel<true>, dim3(n_hi, (unsigned)lv[3]), dim3(SG_NT), 0, s, d_hi, Z);
		}
		if(n_lo)
			hipLaunchKernelGGL(sg_cols_kernel<true>, dim3(n_lo, (unsigned)lv[2]), dim3(SG_NT), lds, s, d_lo, F, Z, rel);
		if(n_hi) {
			hipLaunchKernelGGL(sg_cols_mfma_kernel<true>, dim3(n_hi, (unsigned)lv[4]), dim3(SG_MT), 0, s, d_hi, F, Z);
			hipLaunchKernelGGL(sg_mirror_kernel<false>, dim3(n_hi, (unsigned)lv[4]), dim3(SG_NT), 0, s, d_hi, Z);
		}
	}
	if(ns > 0)
		hipLaunchKernelGGL(sg_gather_kernel, dim3((unsigned)ns), dim3(SG_NT), 0, s, sp->front_off.p, sp->front_w.p, sp->front_ld.p,
			sp->front_pad.p, sp->asm_ptr.p, sp->asm_src.p, sp->asm_dst.p, sp->asm_shape.p, Z, d_sigma);
	SPP_HIP_CHECK(hipGetLastError());
}

} // namespace spp
