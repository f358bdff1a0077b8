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
//                  fused multiply-adds in a fixed order (fs_lds_fwd / fs_lds_bwd of spp_front_subst.h, the bodies of
//                  ss_fwd_kernel / ss_bwd_kernel too);
//   classes 3 - 4  sg_cols_mfma_kernel: sixteen waves, the work columns are the columns of Z themselves, the products are
//                  chains of v_mfma_f64_16x16x4_f64 split over the waves by the front's shape alone and summed in wave
//                  order (fs_mfma_fwd / fs_mfma_bwd, the bodies of ss_fwd_mfma_kernel / ss_bwd_mfma_kernel too); Z21 and
//                  the lower triangle of Z11 are mirrored by launches of their own (sg_mirror_kernel): a column under
//                  work is nobody else's to write.
// The parent is finished by the launch boundary; inside a launch a workgroup reads R, its parent's Z and its own columns
// of Z and writes its own columns (classes 0 - 2: also their mirror rows, which nobody reads before the next launch). No
// flags, no waits. A column of Z meets the same instruction sequence wherever it lands in a tile.

#include "spp_front_subst.h"
#include <algorithm>

namespace spp {

constexpr int SG_NT = FS_NT;        // threads of a workgroup of the LDS body
constexpr int SG_CW = 16;           // columns of Z a workgroup owns
constexpr int SG_MT = FS_MT;        // threads of a workgroup of the MFMA body
// the largest front of class 2 (w = 112, h - 1 = 127): its pivot rows at column stride w | 1 beside 16 work columns
constexpr size_t SG_LDS_MAX = (size_t)(113 * 127 + 127 * SG_CW) * sizeof(double);

// ---- classes 0 - 2 ---------------------------------------------------------------------------------------------------
// PIV = false: the columns w .. h - 2 of Z (steps 1 and 2), PIV = true: the pivot columns (step 3). Dynamic LDS:
// ((w | 1) (h - 1) + 16 (h - 1)) doubles, a launch asks for its largest front's.
template <bool PIV>
__global__ __launch_bounds__(SG_NT)
void sg_cols_kernel(const SigmaFront *__restrict__ desc, const double *__restrict__ fronts, double *zs, const int32_t *__restrict__ rel)
{
	constexpr int CW = SG_CW;
	extern __shared__ double sg_sm[];
	__shared__ double tri[FS_PB * 17];
	__shared__ double ts[FS_PB * CW];
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
	const int tid = threadIdx.x;
	fs_stage_rows(F, ld, w, pad, hc, ws, Rs);
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
	if(PIV)
		fs_lds_fwd<CW>(Rs, ws, w, c0, T, tri, ts); // y = R11^-T e_c from the tile's first column on: the rows above stay zero
	fs_lds_bwd<CW>(Rs, ws, w, hc, T, tri, ts);     // x = R11^-1 (y - R12 t)
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
// where the 16 work columns of a workgroup live: the tile's own columns of Z in the arena (row stride 1, column stride ld,
// first one cbase in the padded image). A tile column beyond the front's last works on a copy of the last one and is never
// stored: no lane reads outside the front.
struct SigmaCols {
	double *Z;
	int ld, pad, cbase, last;
	__device__ double *piv(int p, int j) const { return Z + (int64_t)(cbase + (j < last ? j : last)) * ld + p; }
	__device__ const double *upd(int c, int j) const { return piv(c + pad, j); }
	__device__ double start(int p, int j) const { return *piv(p, j); }
	__device__ bool may_store(int j) const { return j <= last; }
};

// Step 2 finds Z22 in the columns' rows w .. h - 2 (sg_fetch_kernel, the launch before) and clears the pivot rows, step 3
// finds Z21 there and sets e_c.
template <bool PIV>
__global__ __launch_bounds__(SG_MT)
void sg_cols_mfma_kernel(const SigmaFront *__restrict__ desc, const double *__restrict__ fronts, double *zs)
{
	constexpr int CW = SG_CW;
	__shared__ double tri[FS_PB * 17];
	__shared__ double ts[FS_PB * CW];
	__shared__ double part[FS_MW][FS_PB * CW];
	const SigmaFront fd = desc[blockIdx.x];
	const int h = fd.h, w = fd.w, ld = fd.ld, pad = fd.pad;
	const int hc = h - 1, m = hc - w;
	const int ncols = PIV ? w : m;
	const int c0 = (int)blockIdx.y * CW;
	if(c0 >= ncols)
		return;
	const double *F = fronts + fd.off;
	double *Z = zs + fd.off;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int cbase = PIV ? c0 : w + pad + c0;     // first column of the tile in the padded image
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
	const SigmaCols cols{Z, ld, pad, cbase, ncols - 1 - c0};
	if(PIV)
		fs_mfma_fwd(F, ld, w, c0, cols, tri, ts, part); // y = R11^-T e_c from the tile's first column on
	fs_mfma_bwd(F, ld, w, pad, hc, cols, tri, ts, part); // x = R11^-1 (y - R12 t)
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
	sparse_sigma_arena(ctx);
	sparse_sigma_gather(ctx, d_sigma);
}

// steps 1 - 3 down the assembly tree: Z_s of every front into the arena sigma_z
void sparse_sigma_arena(spp_ctx *ctx)
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
	SPP_HIP_CHECK(hipGetLastError());
}

// the assembly map backwards, out of the arena sparse_sigma_arena filled: every stored block of the factored matrix has
// one entry, so every double of dst (the layout of that matrix's value array) is written once
void sparse_sigma_gather(spp_ctx *ctx, double *dst)
{
	SparsePlan *sp = ctx->sparse;
	SPP_REQUIRE(sp && sp->sigma_z.p, SPP_E_STATE, "sparse plan or its arena of Z missing");
	const int64_t ns = sp->n_snodes;
	if(ns > 0)
		hipLaunchKernelGGL(sg_gather_kernel, dim3((unsigned)ns), dim3(SG_NT), 0, ctx->stream, sp->front_off.p, sp->front_w.p,
			sp->front_ld.p, sp->front_pad.p, sp->asm_ptr.p, sp->asm_src.p, sp->asm_dst.p, sp->asm_shape.p, sp->sigma_z.p, dst);
	SPP_HIP_CHECK(hipGetLastError());
}

} // namespace spp
