// spp_sparse_solve.hip -- Lambda X = B for k right-hand sides against the multifrontal factor a sparse solve left behind
// (DESIGN.md section 27); the joint covariance of chosen vertices is kept_marginals (spp_solve_again.hip) on top of it.
//
// After spp_factor_solve_device in the sparse mode every supernode's pivot rows of R (R^T R = P Lambda P^T) sit in the
// plan's `fronts`: R[i, c] = F[i + padded(c, w, pad) * ld], i < w, c < h - 1 (column h - 1 is the right-hand-side slot of
// the factorization and takes no part here). Nothing rewrites them until the next factorization. The forward
// substitution of the factorization rides inside it and cannot be reused, so both substitutions are here:
//     1  Xp <- P B                                                  ss_gather_kernel
//     2  forward, levels ascending: per front
//          t[0:w] = Xp[rows[0:w]], t[w:h-1] = 0, (+) the children's update panels in child_list order through rel,
//          y = R11^-T t[0:w] -> Xp[rows[0:w]], update panel of the front = t[w:h-1] - R12^T y
//     3  backward, levels descending: per front
//          x = R11^-1 (y - R12 Xp[rows[w:h-1]]) -> Xp[rows[0:w]]
//     4  B <- P^T Xp                                                ss_scatter_kernel
// at most 128 columns per pass. Per level and direction one launch for the fronts of classes 0 - 2 and one for those of
// classes 3 - 4: the body is chosen by the front's size class alone, never by k.
//   classes 0 - 2  ss_fwd_kernel / ss_bwd_kernel<CW>: a workgroup owns (front, CW columns), CW = 1 .. 16 by the column count
//                  (who computes an entry, never how); the front's pivot rows and its work vector are staged in LDS, every
//                  entry of a column is ONE chain of explicit fused multiply-adds from LDS in a fixed order (pivots
//                  ascending forward, columns ascending backward);
//   classes 3 - 4  ss_fwd_mfma_kernel / ss_bwd_mfma_kernel: a workgroup of sixteen waves owns (front, 16 columns); the
//                  products in front of a 16-pivot block and the update panel are chains of v_mfma_f64_16x16x4_f64, split
//                  over the waves by the front's shape alone and summed in wave order.
// Children and ancestors live on other levels and are finished by the launch boundary, the fronts of one level own
// disjoint pivot rows and update panels: inside a launch nobody writes what another workgroup reads. No flags, no waits.
// Children are added in list order and no sum meets another column's values: column j of a k-column solve has the bits
// of that column solved alone, whatever k, tile and lane.

// The triangular part of both bodies -- the staging, the block loops, the sweep of the diagonal tile -- is
// spp_front_subst.h's, shared with spp_sparse_sigma.hip; here is what is the solve's own: the permutation, the extend-add
// of the children's panels and the update panel.

#include "spp_front_subst.h"
#include <algorithm>

namespace spp {

constexpr int SS_NT = FS_NT;  // threads of a workgroup: CW columns x 256 / CW rows
constexpr int SS_PASS = 128;  // columns of a pass
constexpr int SS_PB = FS_PB;  // pivots of a block of the triangular solves

struct SolveArgs {
	const int32_t *front_h, *front_w;
	const int32_t *child_list, *rel_ptr, *rel, *rows;
	const int64_t *uoff;   // first row of a front's update panel
	const double *fronts;
	double *xp, *upd;      // xs doubles per row
	int xs, kc;            // row stride of xp / upd, columns of the pass
};

// ---- classes 0 - 2: the front's pivot rows staged in LDS --------------------------------------------------------------
// A workgroup owns (front, CW columns). It stages the w x (h - 1) pivot rows of R once (column stride w | 1) and keeps
// the front's whole work vector t (h - 1 entries per column) beside them: every product chain runs from LDS. Dynamic
// LDS: (ws (h - 1) + (h - 1) CW) doubles, at most 131 KB (w = 112, h - 1 = 127); a launch asks for its largest front's.
constexpr int SS_CH = 32; // children whose descriptors a workgroup caches
constexpr size_t SS_LDS_MAX = (size_t)(113 * 127 + 127 * 16) * sizeof(double);

template <int CW>
__global__ __launch_bounds__(SS_NT)
void ss_fwd_kernel(const AgainFront *__restrict__ desc, SolveArgs a)
{
	constexpr int NR = SS_NT / CW; // rows in flight
	extern __shared__ double ss_sm[];
	__shared__ double tri[SS_PB * 17];
	__shared__ double ts[SS_PB * CW];
	const AgainFront fd = desc[blockIdx.x]; // (one scalar fetch: no walk list -> front -> rows)
	const int h = fd.h, w = fd.w, ld = fd.ld, pad = fd.pad;
	const int hc = h - 1, ws = w | 1;
	double *Rs = ss_sm, *T = ss_sm + ws * hc; // R[i, c] at Rs[i + c * ws]; t[r] of column col at T[r * CW + col]
	const double *F = a.fronts + fd.off;
	const int tid = threadIdx.x, col = tid % CW, q = tid / CW;
	const int c0 = (int)blockIdx.y * CW;
	const bool act = c0 + col < a.kc;
	const int64_t xs = a.xs;
	// (the pivot rows of a supernode are consecutive in the permuted numbering: rows[i] = rows[0] + i, i < w)
	double *X = a.xp + (int64_t)fd.row0 * xs + c0 + col;
	double *U = a.upd + fd.uoff * xs + c0 + col;
	// what the extend-add needs of the first SS_CH children, fetched side by side with the staging: per child one round
	// trip is left (its rows and its panel) instead of three dependent ones
	__shared__ int32_t ch_m[SS_CH], ch_rel[SS_CH];
	__shared__ int64_t ch_u[SS_CH];
	const int cb = fd.cb, ce = fd.ce;
	if(tid < ce - cb && tid < SS_CH) {
		const int c = a.child_list[cb + tid];
		ch_m[tid] = a.front_h[c] - 1 - a.front_w[c];
		ch_rel[tid] = a.rel_ptr[c];
		ch_u[tid] = a.uoff[c];
	}
	fs_stage_rows(F, ld, w, pad, hc, ws, Rs);
	for(int r = q; r < hc; r += NR)
		T[r * CW + col] = (act && r < w) ? X[r * xs] : 0.0; // (a column beyond k is solved on zeros and never stored)
	__syncthreads();
	// ---- extend-add of the children's update panels, children in list order (a child's rows map to distinct rows)
	for(int cq = cb; cq < ce; ++ cq) {
		int mc, relp;
		int64_t uo;
		if(cq - cb < SS_CH) {
			mc = ch_m[cq - cb]; relp = ch_rel[cq - cb]; uo = ch_u[cq - cb];
		} else {
			const int c = a.child_list[cq];
			mc = a.front_h[c] - 1 - a.front_w[c]; relp = a.rel_ptr[c]; uo = a.uoff[c];
		}
		const double *Uc = a.upd + uo * xs + c0 + col;
		const int32_t *rl = a.rel + relp;
		if(act)
			for(int i = q; i < mc; i += NR)
				T[rl[i] * CW + col] += Uc[i * xs];
		__syncthreads();
	}
	fs_lds_fwd<CW>(Rs, ws, w, 0, T, tri, ts); // y = R11^-T t
	// ---- update panel of the front: t[w:h-1] - R12^T y, one chain per entry over all pivots
	for(int r = w + q; r < hc; r += NR) {
		const double *Rc = Rs + r * ws;
		double acc = T[r * CW + col];
		for(int p = 0; p < w; ++ p)
			acc = __builtin_fma(-Rc[p], T[p * CW + col], acc);
		T[r * CW + col] = acc;
	}
	__syncthreads();
	if(act)
		for(int r = q; r < hc; r += NR) {
			if(r < w)
				X[r * xs] = T[r * CW + col];
			else
				U[(r - w) * xs] = T[r * CW + col];
		}
}

template <int CW>
__global__ __launch_bounds__(SS_NT)
void ss_bwd_kernel(const AgainFront *__restrict__ desc, SolveArgs a)
{
	constexpr int NR = SS_NT / CW;
	extern __shared__ double ss_sm[];
	__shared__ double tri[SS_PB * 17];
	__shared__ double ts[SS_PB * CW];
	const AgainFront fd = desc[blockIdx.x]; // (one scalar fetch: no walk list -> front -> rows)
	const int h = fd.h, w = fd.w, ld = fd.ld, pad = fd.pad;
	const int hc = h - 1, ws = w | 1;
	double *Rs = ss_sm, *T = ss_sm + ws * hc;
	const double *F = a.fronts + fd.off;
	const int32_t *rw = a.rows + fd.rowsp;
	const int tid = threadIdx.x, col = tid % CW, q = tid / CW;
	const int c0 = (int)blockIdx.y * CW;
	const bool act = c0 + col < a.kc;
	const int64_t xs = a.xs;
	const double *Xg = a.xp + c0 + col;        // by global permuted row: the ancestors' final x
	double *X = a.xp + (int64_t)fd.row0 * xs + c0 + col;
	fs_stage_rows(F, ld, w, pad, hc, ws, Rs);
	for(int r = q; r < hc; r += NR)
		T[r * CW + col] = act ? (r < w ? X[r * xs] : Xg[(int64_t)rw[r] * xs]) : 0.0;
	__syncthreads();
	fs_lds_bwd<CW>(Rs, ws, w, hc, T, tri, ts); // x = R11^-1 (y - R12 t)
	if(act)
		for(int r = q; r < w; r += NR)
			X[r * xs] = T[r * CW + col];
}

// ---- classes 3 - 4: the products on v_mfma_f64_16x16x4_f64 -----------------------------------------------------------
// A workgroup (sixteen waves) owns (front, 16 columns); the work columns are the rows of xp themselves. The update panel
// goes by 16-row tiles, a wave per tile, one chain over all pivots. Rows and columns beyond w / h - 1 are the next
// front's, or nobody's: masked as in spp_front_subst.h.
constexpr int SS_MT = FS_MT;      // threads of a workgroup of the MFMA body
constexpr int SS_MW = FS_MW;      // its waves

// where the 16 work columns of a workgroup live: rows of xp (stride xs), the tile's columns side by side; the update rows
// through the front's row list. Columns beyond kc are allocated (xs is a multiple of 16) and hold nothing.
struct SolveCols {
	double *xg;          // row 0 of xp, the tile's first column: rows by their global permuted number
	int row0;            // the front's first pivot row
	const int32_t *rw;   // the front's rows
	int xs, kc0;         // row stride, columns of the pass from the tile's first on
	__device__ SolveCols(const SolveArgs &a, const AgainFront &fd, int c0)
		: xg(a.xp + c0), row0(fd.row0), rw(a.rows + fd.rowsp), xs(a.xs), kc0(a.kc - c0) {}
	__device__ double *piv(int p, int j) const { return xg + (int64_t)(row0 + p) * xs + j; }
	__device__ const double *upd(int c, int j) const { return xg + (int64_t)rw[c] * xs + j; }
	__device__ double start(int p, int j) const { return may_store(j) ? *piv(p, j) : 0.0; }
	__device__ bool may_store(int j) const { return j < kc0; }
};

__global__ __launch_bounds__(SS_MT)
void ss_fwd_mfma_kernel(const AgainFront *__restrict__ desc, SolveArgs a)
{
	constexpr int CW = 16, NR = SS_MT / CW;
	__shared__ double tri[SS_PB * 17];
	__shared__ double ts[SS_PB * CW];
	__shared__ double part[SS_MW][SS_PB * CW];
	const AgainFront fd = desc[blockIdx.x]; // (one scalar fetch: no walk list -> front -> rows)
	const int h = fd.h, w = fd.w, ld = fd.ld, pad = fd.pad;
	const int m = h - 1 - w;
	const double *F = a.fronts + fd.off;
	const int tid = threadIdx.x, col = tid % CW, q = tid / CW;
	const int lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
	const int c0 = (int)blockIdx.y * CW;
	const bool act = c0 + col < a.kc;
	const int64_t xs = a.xs;
	double *X = a.xp + (int64_t)fd.row0 * xs + c0 + col;
	double *U = a.upd + fd.uoff * xs + c0 + col;
	const double *Xb = a.xp + (int64_t)fd.row0 * xs + c0 + l15; // B operand: y[p][column l15 of the tile]
	if(act)
		for(int i = q; i < m; i += NR)
			U[i * xs] = 0.0;
	__syncthreads();
	for(int cq = fd.cb; cq < fd.ce; ++ cq) {
		const int c = a.child_list[cq];
		const int mc = a.front_h[c] - 1 - a.front_w[c];
		const double *Uc = a.upd + a.uoff[c] * xs + c0 + col;
		const int32_t *rl = a.rel + a.rel_ptr[c];
		if(act)
			for(int i = q; i < mc; i += NR) {
				const int d = rl[i];
				const double v = Uc[i * xs];
				if(d < w)
					X[d * xs] += v;
				else
					U[(d - w) * xs] += v;
			}
		__syncthreads();
	}
	fs_mfma_fwd(F, ld, w, 0, SolveCols(a, fd, c0), tri, ts, part); // y = R11^-T t
	// ---- update panel -= R12^T y, a wave per tile of 16 rows
	for(int i0 = wave * SS_PB; i0 < m; i0 += SS_MW * SS_PB) {
		v4f64 acc = (v4f64){0, 0, 0, 0};
		const bool ci = i0 + l15 < m;
		for(int p0 = 0; p0 < w; p0 += SS_PB) {
			const double *pa[4], *pb[4];
#pragma unroll
			for(int kk = 0; kk < 4; ++ kk) {
				const int p = p0 + 4 * kk + l4;
				pa[kk] = (ci && p < w) ? F + p + (int64_t)(w + pad + i0 + l15) * ld : &fs_zero_word;
				pb[kk] = p < w ? Xb + p * xs : &fs_zero_word;
			}
			acc = fs_mfma16(pa, pb, acc);
		}
		if(c0 + l15 < a.kc) {
			double *Ul = a.upd + fd.uoff * xs + c0 + l15;
#pragma unroll
			for(int r = 0; r < 4; ++ r) {
				const int i = i0 + l4 + 4 * r;
				if(i < m)
					Ul[i * xs] -= acc[r];
			}
		}
	}
}

__global__ __launch_bounds__(SS_MT)
void ss_bwd_mfma_kernel(const AgainFront *__restrict__ desc, SolveArgs a)
{
	constexpr int CW = 16;
	__shared__ double tri[SS_PB * 17];
	__shared__ double ts[SS_PB * CW];
	__shared__ double part[SS_MW][SS_PB * CW];
	const AgainFront fd = desc[blockIdx.x]; // (one scalar fetch: no walk list -> front -> rows)
	// x = R11^-1 (y - R12 x of the ancestors, by global permuted row)
	fs_mfma_bwd(a.fronts + fd.off, fd.ld, fd.w, fd.pad, fd.h - 1, SolveCols(a, fd, (int)blockIdx.y * CW), tri, ts, part);
}

// Xp[i, j] = B[perm[i], j], a thread per (row, column of the pass)
__global__ __launch_bounds__(SS_NT)
void ss_gather_kernel(int64_t n, int kc, int xs, const int32_t *__restrict__ perm, const double *__restrict__ B, int64_t ldb,
	double *__restrict__ xp)
{
	const int64_t e = (int64_t)blockIdx.x * SS_NT + threadIdx.x;
	const int64_t i = e / kc;
	const int j = (int)(e % kc);
	if(i < n)
		xp[i * xs + j] = B[perm[i] + j * ldb];
}

__global__ __launch_bounds__(SS_NT)
void ss_scatter_kernel(int64_t n, int kc, int xs, const int32_t *__restrict__ perm, const double *__restrict__ xp,
	double *__restrict__ B, int64_t ldb)
{
	const int64_t e = (int64_t)blockIdx.x * SS_NT + threadIdx.x;
	const int64_t i = e / kc;
	const int j = (int)(e % kc);
	if(i < n)
		B[perm[i] + j * ldb] = xp[i * xs + j];
}

// per level two launches at most: the fronts of classes 0 - 2 (plain body, CW columns per workgroup) and those of classes
// 3 - 4 (MFMA body, 16 columns per workgroup); the body is chosen by the front's class alone, never by k
template <int CW>
static void ss_levels(SparsePlan *sp, hipStream_t s, const SolveArgs &a, unsigned tiles, unsigned tiles16)
{
	static uint64_t attr_seen = 0;
	if(first_on_this_device(attr_seen)) {
		SPP_HIP_CHECK(hipFuncSetAttribute((const void*)ss_fwd_kernel<CW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SS_LDS_MAX));
		SPP_HIP_CHECK(hipFuncSetAttribute((const void*)ss_bwd_kernel<CW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SS_LDS_MAX));
	}
	// dynamic LDS of a level's class 0 - 2 launch: the staged rows of its largest front and the work vectors of its tallest
	auto lds = [&](int64_t l) { return (size_t)(sp->h_again_rmax[l] + sp->h_again_hmax[l] * CW) * sizeof(double); };
	for(int64_t l = 0; l < sp->n_levels; ++ l) {
		const int32_t *cp = sp->h_cls_ptr.data() + l * NCLS;
		if(cp[3] > cp[0])
			hipLaunchKernelGGL((ss_fwd_kernel<CW>), dim3((unsigned)(cp[3] - cp[0]), tiles), dim3(SS_NT), lds(l), s, sp->again_desc.p + cp[0], a);
		if(cp[5] > cp[3])
			hipLaunchKernelGGL(ss_fwd_mfma_kernel, dim3((unsigned)(cp[5] - cp[3]), tiles16), dim3(SS_MT), 0, s, sp->again_desc.p + cp[3], a);
	}
	for(int64_t l = sp->n_levels; l > 0;) {
		-- l;
		const int32_t *cp = sp->h_cls_ptr.data() + l * NCLS;
		if(cp[3] > cp[0])
			hipLaunchKernelGGL((ss_bwd_kernel<CW>), dim3((unsigned)(cp[3] - cp[0]), tiles), dim3(SS_NT), lds(l), s, sp->again_desc.p + cp[0], a);
		if(cp[5] > cp[3])
			hipLaunchKernelGGL(ss_bwd_mfma_kernel, dim3((unsigned)(cp[5] - cp[3]), tiles16), dim3(SS_MT), 0, s, sp->again_desc.p + cp[3], a);
	}
}

void sparse_solve_again(spp_ctx *ctx, double *d_B, int64_t ldb, int64_t nrhs)
{
	SparsePlan *sp = ctx->sparse;
	SPP_REQUIRE(sp, SPP_E_STATE, "sparse plan missing");
	hipStream_t s = ctx->stream;
	const int64_t ns = sp->n_snodes, n = sp->n;
	if(sp->h_again_uoff.empty()) { // (the host image lives in the plan: its upload may still run when this call returns)
		sp->h_again_uoff.resize((size_t)ns);
		int64_t r = 0;
		for(int64_t q = 0; q < ns; ++ q) {
			sp->h_again_uoff[q] = r;
			r += sp->h_front_h[q] - 1 - sp->h_front_w[q];
		}
		sp->again_urows = r;
		sp->h_again_rmax.assign((size_t)sp->n_levels, 0);
		sp->h_again_hmax.assign((size_t)sp->n_levels, 0);
		for(int64_t l = 0; l < sp->n_levels; ++ l)
			for(int32_t i = sp->h_cls_ptr[l * NCLS]; i < sp->h_cls_ptr[l * NCLS + 3]; ++ i) { // the level's fronts of classes 0 - 2
				const int32_t f = sp->h_level_fronts[i], hc = sp->h_front_h[f] - 1, w = sp->h_front_w[f];
				sp->h_again_rmax[l] = std::max(sp->h_again_rmax[l], (w | 1) * hc);
				sp->h_again_hmax[l] = std::max(sp->h_again_hmax[l], hc);
			}
		sp->again_uoff.upload(sp->h_again_uoff, s);
		// one descriptor per front, in the order of level_fronts: a workgroup finds everything about its front in one fetch
		{
			std::vector<int64_t> row0((size_t)ns), rowsp((size_t)ns);
			int64_t r0 = 0, rp = 0;
			for(int64_t q = 0; q < ns; ++ q) { // (supernodes are consecutive pivot ranges of the permuted numbering; rows_ptr sums h)
				row0[q] = r0; rowsp[q] = rp;
				r0 += sp->h_front_w[q]; rp += sp->h_front_h[q];
			}
			sp->h_again_desc.resize((size_t)ns);
			for(int64_t i = 0; i < ns; ++ i) {
				const int32_t f = sp->h_level_fronts[i];
				AgainFront &d = sp->h_again_desc[i];
				d.off = sp->h_front_off[f]; d.uoff = sp->h_again_uoff[f];
				d.h = sp->h_front_h[f]; d.w = sp->h_front_w[f]; d.ld = sp->h_front_ld[f]; d.pad = sp->h_front_pad[f];
				d.row0 = (int32_t)row0[f]; d.rowsp = (int32_t)rowsp[f];
				d.cb = sp->h_child_ptr[f]; d.ce = sp->h_child_ptr[f + 1];
			}
			sp->again_desc.upload(sp->h_again_desc, s);
		}
		// both panels once, for a full pass of 128 columns: no later call allocates, whatever its k
		sp->again_xp.reserve((size_t)n * SS_PASS);
		sp->again_upd.reserve((size_t)std::max<int64_t>(sp->again_urows, 1) * SS_PASS);
	}
	for(int64_t k0 = 0; k0 < nrhs; k0 += SS_PASS) {
		const int kc = (int)std::min<int64_t>(SS_PASS, nrhs - k0);
		int cw = 1;
		while(cw < 16 && cw < kc)
			cw *= 2;
		const unsigned tiles = (unsigned)((kc + cw - 1) / cw);
		int nct = 1; // tiles of 16 columns a row of the panels holds: 1, 2, 4, 8
		while(16 * nct < kc)
			nct *= 2;
		const int xs = 16 * nct; // (the MFMA body reads whole tiles of 16 columns)
		const unsigned tiles16 = (unsigned)((kc + 15) / 16);
		SolveArgs a;
		a.front_h = sp->front_h.p; a.front_w = sp->front_w.p;
		a.child_list = sp->child_list.p; a.rel_ptr = sp->rel_ptr.p; a.rel = sp->rel.p; a.rows = sp->rows.p;
		a.uoff = sp->again_uoff.p;
		a.fronts = sp->fronts.p;
		a.xp = sp->again_xp.p; a.upd = sp->again_upd.p;
		a.xs = xs; a.kc = kc;
		double *B = d_B + k0 * ldb;
		const unsigned gn = (unsigned)((n * kc + SS_NT - 1) / SS_NT);
		hipLaunchKernelGGL(ss_gather_kernel, dim3(gn), dim3(SS_NT), 0, s, n, kc, xs, sp->perm_scalar.p, B, ldb, sp->again_xp.p);
		switch(cw) {
		case 1: ss_levels<1>(sp, s, a, tiles, tiles16); break;
		case 2: ss_levels<2>(sp, s, a, tiles, tiles16); break;
		case 4: ss_levels<4>(sp, s, a, tiles, tiles16); break;
		case 8: ss_levels<8>(sp, s, a, tiles, tiles16); break;
		default: ss_levels<16>(sp, s, a, tiles, tiles16); break;
		}
		hipLaunchKernelGGL(ss_scatter_kernel, dim3(gn), dim3(SS_NT), 0, s, n, kc, xs, sp->perm_scalar.p, sp->again_xp.p, B, ldb);
	}
	SPP_HIP_CHECK(hipGetLastError());
}

} // namespace spp
