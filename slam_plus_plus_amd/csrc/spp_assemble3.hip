// spp_assemble3.hip -- Lambda and eta of TERNARY edges on gfx950, fp64: self-calibrating bundle adjustment, one residual
// of CEdgeP2CI3D feeding a camera (6), a point (3) and an intrinsics vertex (5, stored 6 wide with one inert coordinate).
//
// Replaces, for an n-ary edge,
//   symbolic: Alloc_HessianBlocks_v2 (reference include/slam/BaseTypes.h:1540-1767): one upper block per pair of the edge's
//             vertices, transposed when the ids are reversed
//   numeric : Calculate_Hessians_v2 (:1981-2130) + the reduction plan (NonlinearSolver_Lambda_Base.h:563-607, 152-197), the
//             unary factor (:1903-1924) and the Levenberg-Marquardt damping (NonlinearSolver_Lambda_LM.h:228-239).
//
// What an edge gives to H00, H01, H11, g0, g1 is exactly what the (6,3,2) binary edge gives: the plan holds an ordinary
// binary plan over (camera, point) whose offsets point into the union structure, and assemble_run() writes those
// destinations with the kernels of spp_assemble.hip, bit for bit. The BORDER kernels here write every destination that
// touches an intrinsics vertex: H02 per (camera, intrinsics) pair, H12 per (point, intrinsics) pair, H22 and g2 per
// intrinsics vertex. An intrinsics vertex is in none of the binary lists; its diagonal block and eta segment are written
// here, with the unary factor (identity on the 5 live coordinates), the damping and 1.0 on the inert diagonal entry.
//
// An intrinsics vertex is a HUB: it is touched by every observation of its cameras (10^3 .. 10^6), and so is its block
// against each camera (Venice: 871 blocks of about 3 260 terms, 2 838 740 / 871). One thread or one wave per destination would run these as
// one long serial loop, so a destination is summed in one of two ways, by its number of edges alone:
//   <= SEQ_MAX_DEGREE (24)  border_seq_kernel: one thread, edge order, first assigned, the rest added
//   longer                  the edge list is cut into chunks of ASM_HUB_CHUNK (C = 4096) positions;
//       stage 1  hub_chunk_kernel: ONE workgroup of 256 threads per chunk. Thread t sums the positions t, t + 256, ... of
//                its chunk in ascending order (at most C / 256 = 16 terms), the 64 lanes of a wave are summed by the
//                xor butterfly (32, 16, 8, 4, 2, 1: 6 additions), the 4 waves through LDS in ascending order
//                (3 additions); the partial goes to its slot
//       stage 2  hub_final_kernel: one lane per value adds the destination's partials in ascending chunk order and
//                stores the block (transposed if need be; diagonal: mirrored, unary factor, damping, inert 1.0)
//   The tree is fixed by C and by the 256 threads of stage 1, which are constants of the code: the bits of the result do not
//   depend on the grid, on the number of CUs, on which workgroup runs first, or on the run. A term passes through at most
//   (C / 256 - 1) + 6 + 3 + (chunks - 1) additions.
// Stage 1 is HBM-bound like the binary kernels: an edge's J0 / J1 / J2 / Omega / r (12 + 6 + 12 + 4 + 2 doubles) are read
// once per destination they feed; 256 CUs x one workgroup of 4 waves, <= 36 accumulators per thread, 1.2 KB of LDS.

#include "spp_assemble_plan.h"
#include <algorithm>
#include <cstdint>

namespace spp {

static const int HUB_THREADS = 256;  // the workgroup of stage 1: part of the reduction tree, not a tuning knob
static const int HUB_STRIDE = 36;    // doubles per partial slot: the widest destination (H02: 6 x 6)

// --------------------------------------------------------------------------------------------------
// analysis (host)
// --------------------------------------------------------------------------------------------------
namespace {

struct KeyedEdge {
	int64_t a, b; // destination: (intrinsics, other vertex)
	int32_t e;
	bool operator<(const KeyedEdge &o) const { return a != o.a ? a < o.a : b != o.b ? b < o.b : e < o.e; }
};

// offset of the upper block (row, col) in a structure
int64_t block_offset(const Structure &st, int64_t row, int64_t col)
{
	const int64_t *b = st.row_idx.data() + st.col_ptr[col], *e = st.row_idx.data() + st.col_ptr[col + 1];
	const int64_t *p = std::lower_bound(b, e - 1, row); // (the diagonal block is last)
	SPP_REQUIRE(p < e && *p == row, SPP_E_STATE, "ternary plan: block missing from the union structure");
	return st.blk_off[p - st.row_idx.data()];
}

} // namespace

void assemble_analyze_ternary(spp_ctx *ctx, int64_t nv, const int32_t *dim, int64_t ne, const int64_t *v0, const int64_t *v1,
	const int64_t *v2, int64_t unary_vertex)
{
	assemble_release(ctx); // after a rejected call the ctx has NO assembly plan
	SPP_REQUIRE(ne < (int64_t(1) << 30) / 3, SPP_E_UNSUPPORTED, "too many edges for 31-bit list positions");
	SPP_REQUIRE(unary_vertex < nv, SPP_E_BADARG, "unary_vertex out of range");
	std::vector<uint8_t> is_intr(nv, 0), is_cam(nv, 0);
	for(int64_t e = 0; e < ne; ++ e) {
		const int64_t a = v0[e], b = v1[e], c = v2[e];
		SPP_REQUIRE(a >= 0 && a < nv && b >= 0 && b < nv && c >= 0 && c < nv, SPP_E_BADARG, "bad edge");
		SPP_REQUIRE(a != b && a != c && b != c, SPP_E_BADARG, "two equal vertices in one edge");
		SPP_REQUIRE(dim[a] == 6 && dim[b] == 3 && dim[c] == 6, SPP_E_BADARG, "vertex width does not match the edge shape (6,3,6)");
		is_cam[a] = 1;
		is_intr[c] = 1;
	}
	for(int64_t v = 0; v < nv; ++ v)
		SPP_REQUIRE(!(is_cam[v] && is_intr[v]), SPP_E_BADARG, "a vertex is the camera of one edge and the intrinsics of another");
	VClock clk("assemble_analyze_ternary");
	// ---- the (camera, point) part: an ordinary (6,3,2) plan without the intrinsics vertices in its lists
	const int d0 = 6, d1 = 3, rd = 2;
	const bool unary_intr = unary_vertex >= 0 && is_intr[unary_vertex];
	// (assemble_analyze describes the BINARY structure in the ctx and judges the solver's plan by it; what counts is the
	// union structure: the ctx's sizes and mode are put back here and settled at the end -- analysing the same ternary
	// graph again keeps the solver's symbolic analysis)
	struct Drop {
		spp_ctx *c; bool keep; int mode; int64_t nb, n, nnzb, nvals;
		void put_back() { c->mode = mode; c->st.nb = nb; c->st.n = n; c->st.nnzb = nnzb; c->st.nvals = nvals; }
		~Drop() { if(!keep) { assemble_release(c); put_back(); } }
	} drop = {ctx, false, ctx->mode, ctx->st.nb, ctx->st.n, ctx->st.nnzb, ctx->st.nvals};
	assemble_analyze(ctx, nv, dim, 1, &ne, &v0, &v1, nullptr, &d0, &d1, &rd, unary_intr ? -1 : unary_vertex, is_intr.data());
	drop.put_back();
	AssemblePlan *ap = ctx->assemble;
	clk.lap("binary part");
	// ---- destinations of the border, kind by kind, each with its edges in ascending order
	std::vector<KeyedEdge> k02(ne), k12(ne), k22(ne);
	for(int64_t e = 0; e < ne; ++ e) {
		k02[e] = KeyedEdge{v2[e], v0[e], (int32_t)e};
		k12[e] = KeyedEdge{v2[e], v1[e], (int32_t)e};
		k22[e] = KeyedEdge{v2[e], v2[e], (int32_t)e};
	}
	std::sort(k02.begin(), k02.end());
	std::sort(k12.begin(), k12.end());
	std::sort(k22.begin(), k22.end());
	const std::vector<KeyedEdge> *keyed[3] = {&k02, &k12, &k22};
	std::vector<int32_t> dst_ptr(1, 0), dst_edge;
	std::vector<int64_t> dst_a, dst_b; // (intrinsics, other) of every destination
	int64_t kind_beg[4] = {0};
	dst_edge.reserve(3 * ne);
	for(int k = 0; k < 3; ++ k) {
		const std::vector<KeyedEdge> &ke = *keyed[k];
		for(int64_t q = 0; q < ne; ++ q) {
			if(q && (ke[q].a != ke[q - 1].a || ke[q].b != ke[q - 1].b))
				dst_ptr.push_back((int32_t)dst_edge.size());
			if(!q || ke[q].a != ke[q - 1].a || ke[q].b != ke[q - 1].b) {
				dst_a.push_back(ke[q].a);
				dst_b.push_back(ke[q].b);
			}
			dst_edge.push_back(ke[q].e);
		}
		if(ne)
			dst_ptr.push_back((int32_t)dst_edge.size());
		kind_beg[k + 1] = (int64_t)dst_a.size();
	}
	const int64_t n_dst = kind_beg[3];
	clk.lap("border lists");
	// ---- union structure: the blocks of the binary part + one per (camera, intrinsics) and (point, intrinsics) pair
	const Structure &bs = ap->st;
	Structure us;
	us.nb = nv; us.n = bs.n; us.dim = bs.dim; us.base = bs.base;
	us.col_ptr.assign(nv + 1, 0);
	for(int64_t c = 0; c < nv; ++ c)
		us.col_ptr[c + 1] = bs.col_ptr[c + 1] - bs.col_ptr[c];
	for(int64_t d = 0; d < kind_beg[2]; ++ d)
		++ us.col_ptr[std::max(dst_a[d], dst_b[d]) + 1];
	for(int64_t c = 0; c < nv; ++ c)
		us.col_ptr[c + 1] += us.col_ptr[c];
	us.nnzb = us.col_ptr[nv];
	us.row_idx.resize(us.nnzb);
	us.blk_off.resize(us.nnzb);
	{
		std::vector<int64_t> fill(us.col_ptr.begin(), us.col_ptr.end() - 1);
		for(int64_t c = 0; c < nv; ++ c)
			for(int64_t p = bs.col_ptr[c]; p < bs.col_ptr[c + 1] - 1; ++ p)
				us.row_idx[fill[c] ++] = bs.row_idx[p];
		for(int64_t d = 0; d < kind_beg[2]; ++ d)
			us.row_idx[fill[std::max(dst_a[d], dst_b[d])] ++] = std::min(dst_a[d], dst_b[d]);
		int64_t off = 0;
		for(int64_t c = 0; c < nv; ++ c) {
			SPP_REQUIRE(fill[c] == us.col_ptr[c + 1] - 1, SPP_E_STATE, "ternary plan: column count");
			std::sort(us.row_idx.begin() + us.col_ptr[c], us.row_idx.begin() + fill[c]);
			us.row_idx[fill[c]] = c; // diagonal block last
			for(int64_t p = us.col_ptr[c]; p < us.col_ptr[c + 1]; ++ p) {
				us.blk_off[p] = off;
				off += (int64_t)dim[us.row_idx[p]] * dim[c];
			}
		}
		us.nvals = off;
	}
	clk.lap("union structure");
	// ---- the binary plan's offsets, re-aimed at the union structure
	std::vector<int64_t> ob_off((size_t)ap->n_ob), v_doff(nv);
	{
		int64_t k = 0;
		for(int64_t c = 0; c < nv; ++ c) {
			for(int64_t p = bs.col_ptr[c]; p < bs.col_ptr[c + 1] - 1; ++ p)
				ob_off[k ++] = block_offset(us, bs.row_idx[p], c);
			v_doff[c] = us.blk_off[us.col_ptr[c + 1] - 1];
		}
		SPP_REQUIRE(k == ap->n_ob, SPP_E_STATE, "ternary plan: off-diagonal block count");
	}
	// ---- border destinations: offsets, flags, sequential / hub lists
	struct Guard { TernaryPlan *p; ~Guard() { delete p; } } guard = {new TernaryPlan};
	TernaryPlan *tp = guard.p;
	std::vector<int64_t> dst_off(n_dst), dst_eoff(n_dst, 0);
	std::vector<int32_t> dst_flags(n_dst, 0);
	std::vector<int32_t> seq[3], ch_dst[3], ch_beg[3], ch_slot[3], hub_dst, hub_kind, hub_slot_ptr(1, 0);
	int64_t n_slots = 0;
	for(int k = 0; k < 3; ++ k) {
		for(int64_t d = kind_beg[k]; d < kind_beg[k + 1]; ++ d) {
			const int64_t a = dst_a[d], b = dst_b[d];
			if(k == TernaryPlan::K22) {
				dst_off[d] = v_doff[a];
				dst_eoff[d] = us.base[a];
				dst_flags[d] = (a == unary_vertex) ? 1 : 0;
			} else {
				dst_off[d] = block_offset(us, std::min(a, b), std::max(a, b));
				dst_flags[d] = (a < b) ? 1 : 0; // the intrinsics vertex gives the block's ROWS: stored transposed
			}
			const int32_t beg = dst_ptr[d], end = dst_ptr[d + 1];
			if(end - beg <= SEQ_MAX_DEGREE) {
				seq[k].push_back((int32_t)d);
				continue;
			}
			hub_dst.push_back((int32_t)d);
			hub_kind.push_back(k);
			for(int32_t q = beg; q < end; q += ASM_HUB_CHUNK) {
				ch_dst[k].push_back((int32_t)d);
				ch_beg[k].push_back(q);
				ch_slot[k].push_back((int32_t)n_slots ++);
			}
			hub_slot_ptr.push_back((int32_t)n_slots);
		}
	}
	tp->n_dst = n_dst;
	tp->n_chunks = n_slots;
	tp->n_hub = (int64_t)hub_dst.size();
	hipStream_t s = ctx->stream;
	UploadArena arena(s);
	arena.add(tp->dst_ptr, dst_ptr);
	arena.add(tp->dst_edge, dst_edge);
	arena.add(tp->dst_off, dst_off);
	arena.add(tp->dst_eoff, dst_eoff);
	arena.add(tp->dst_flags, dst_flags);
	for(int k = 0; k < 3; ++ k) {
		tp->n_seq[k] = (int64_t)seq[k].size();
		tp->n_chunk[k] = (int64_t)ch_dst[k].size();
		arena.add(tp->seq_list[k], seq[k]);
		arena.add(tp->chunk_dst[k], ch_dst[k]);
		arena.add(tp->chunk_beg[k], ch_beg[k]);
		arena.add(tp->chunk_slot[k], ch_slot[k]);
	}
	arena.add(tp->hub_dst, hub_dst);
	arena.add(tp->hub_kind, hub_kind);
	arena.add(tp->hub_slot_ptr, hub_slot_ptr);
	arena.commit(tp->index_store);
	tp->partial.reserve((size_t)std::max<int64_t>(n_slots, 1) * HUB_STRIDE);
	if(ap->n_ob)
		SPP_HIP_CHECK(hipMemcpyAsync(ap->ob_off.p, ob_off.data(), ob_off.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
	SPP_HIP_CHECK(hipMemcpyAsync(ap->v_doff.p, v_doff.data(), v_doff.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
	SPP_HIP_CHECK(hipStreamSynchronize(s));
	clk.lap("uploads");
	// complete: the plan now describes the union structure
	ap->st = std::move(us);
	const Structure &st = ap->st;
	if(ctx->mode >= 0 && (ctx->st.nb != st.nb || ctx->st.n != st.n || ctx->st.nnzb != st.nnzb || ctx->st.nvals != st.nvals))
		ctx->mode = -1;
	ctx->st.nb = st.nb; ctx->st.n = st.n; ctx->st.nnzb = st.nnzb; ctx->st.nvals = st.nvals;
	ap->ternary = tp;
	guard.p = nullptr;
	drop.keep = true;
}

// --------------------------------------------------------------------------------------------------
// device
// --------------------------------------------------------------------------------------------------
template <int KIND> struct BorderShape;
template <> struct BorderShape<TernaryPlan::K02> { enum { NV = 36 }; }; // (J0^T Omega J2)(i, c) at i + 6 c
template <> struct BorderShape<TernaryPlan::K12> { enum { NV = 18 }; }; // (J1^T Omega J2)(i, c) at i + 3 c
template <> struct BorderShape<TernaryPlan::K22> { enum { NV = 27 }; }; // upper J2^T Omega J2 (i <= c) at c (c + 1) / 2 + i, then g2 at 21 + i

// the term of one edge for a destination of the kind
template <int KIND>
__device__ __forceinline__ void border_term(int64_t e, const double *__restrict__ J0, const double *__restrict__ J1,
	const double *__restrict__ J2, const double *__restrict__ Om, const double *__restrict__ r, double *v)
{
	double om[4], j2[12];
#pragma unroll
	for(int i = 0; i < 4; ++ i) om[i] = Om[e * 4 + i];
#pragma unroll
	for(int i = 0; i < 12; ++ i) j2[i] = J2[e * 12 + i];
	if(KIND == TernaryPlan::K22) {
		double rr[2], H[36], g[6];
		rr[0] = r[e * 2]; rr[1] = r[e * 2 + 1];
		vertex_contrib<6, 2, 1>(j2, om, rr, 1.0, H, g); // as the second vertex of a binary edge: J^T Omega J, J^T (Omega r)
#pragma unroll
		for(int c = 0; c < 6; ++ c)
#pragma unroll
			for(int i = 0; i <= c; ++ i) v[c * (c + 1) / 2 + i] = H[i + c * 6];
#pragma unroll
		for(int i = 0; i < 6; ++ i) v[21 + i] = g[i];
	} else {
		constexpr int DA = (KIND == TernaryPlan::K02) ? 6 : 3;
		const double *__restrict__ JA = (KIND == TernaryPlan::K02) ? J0 : J1;
		double ja[2 * DA], T[2 * DA];
#pragma unroll
		for(int i = 0; i < 2 * DA; ++ i) ja[i] = JA[e * 2 * DA + i];
		jt_omega<DA, 2>(ja, om, T);
#pragma unroll
		for(int c = 0; c < 6; ++ c)
#pragma unroll
			for(int i = 0; i < DA; ++ i)
				v[i + c * DA] = T[i] * j2[2 * c] + T[i + DA] * j2[2 * c + 1];
	}
}

// stores the finished sum of destination d
template <int KIND>
__device__ __forceinline__ void border_store_value(int k, double x, int32_t flags, double damping, double *__restrict__ o,
	double *__restrict__ eo)
{
	if(KIND == TernaryPlan::K02) {
		const int i = k % 6, c = k / 6;
		o[(flags & 1) ? (c + 6 * i) : (i + 6 * c)] = x;
	} else if(KIND == TernaryPlan::K12) {
		const int i = k % 3, c = k / 3;
		o[(flags & 1) ? (c + 6 * i) : (i + 3 * c)] = x;
	} else if(k >= 21)
		eo[k - 21] = x;
	else {
		int c = 0;
		while((c + 1) * (c + 2) / 2 <= k)
			++ c;
		const int i = k - c * (c + 1) / 2;
		if(i == c) {
			if(c == 5)
				x += 1.0;          // the inert coordinate: its row and column are exact zeros otherwise
			else if(flags & 1)
				x += 1.0;          // unary factor: the identity on the live coordinates
			x += damping;
		}
		o[i + 6 * c] = x;
		o[c + 6 * i] = x;
	}
}

template <int KIND>
__global__ __launch_bounds__(256)
void border_seq_kernel(int64_t n, const int32_t *__restrict__ list, const int32_t *__restrict__ dst_ptr,
	const int32_t *__restrict__ dst_edge, const int64_t *__restrict__ dst_off, const int64_t *__restrict__ dst_eoff,
	const int32_t *__restrict__ dst_flags, const double *__restrict__ J0, const double *__restrict__ J1,
	const double *__restrict__ J2, const double *__restrict__ Om, const double *__restrict__ r, double damping,
	double *__restrict__ vals, double *__restrict__ eta)
{
	constexpr int NV = BorderShape<KIND>::NV;
	const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(t >= n)
		return;
	const int32_t d = list[t];
	double acc[NV];
#pragma unroll
	for(int i = 0; i < NV; ++ i) acc[i] = 0;
	bool first = true;
	for(int32_t q = dst_ptr[d]; q < dst_ptr[d + 1]; ++ q) {
		double v[NV];
		border_term<KIND>(dst_edge[q], J0, J1, J2, Om, r, v);
#pragma unroll
		for(int i = 0; i < NV; ++ i) acc[i] = first ? v[i] : acc[i] + v[i]; // first assigned, the rest added
		first = false;
	}
	const int32_t flags = dst_flags[d];
	double *o = vals + dst_off[d], *eo = eta + dst_eoff[d];
#pragma unroll
	for(int k = 0; k < NV; ++ k)
		border_store_value<KIND>(k, acc[k], flags, damping, o, eo);
}

// stage 1 of the hub reduction: one workgroup of HUB_THREADS per chunk
template <int KIND>
__global__ __launch_bounds__(256)
void hub_chunk_kernel(const int32_t *__restrict__ chunk_dst, const int32_t *__restrict__ chunk_beg,
	const int32_t *__restrict__ chunk_slot, const int32_t *__restrict__ dst_ptr, const int32_t *__restrict__ dst_edge,
	const double *__restrict__ J0, const double *__restrict__ J1, const double *__restrict__ J2, const double *__restrict__ Om,
	const double *__restrict__ r, double *__restrict__ partial)
{
	constexpr int NV = BorderShape<KIND>::NV;
	__shared__ double red[HUB_THREADS / 64][NV];
	const int ch = blockIdx.x, tid = threadIdx.x;
	const int32_t beg = chunk_beg[ch], end = min(beg + ASM_HUB_CHUNK, dst_ptr[chunk_dst[ch] + 1]);
	double acc[NV];
#pragma unroll
	for(int i = 0; i < NV; ++ i) acc[i] = 0;
	for(int32_t q = beg + tid; q < end; q += HUB_THREADS) { // ascending positions
		double v[NV];
		border_term<KIND>(dst_edge[q], J0, J1, J2, Om, r, v);
#pragma unroll
		for(int i = 0; i < NV; ++ i) acc[i] += v[i];
	}
#pragma unroll
	for(int i = 0; i < NV; ++ i) {
		double x = acc[i];
#pragma unroll
		for(int off = 32; off > 0; off >>= 1)
			x += __shfl_xor(x, off);
		acc[i] = x;
	}
	if((tid & 63) == 0) {
#pragma unroll
		for(int i = 0; i < NV; ++ i) red[tid >> 6][i] = acc[i];
	}
	__syncthreads();
	if(tid < NV) {
		double x = red[0][tid];
#pragma unroll
		for(int w = 1; w < HUB_THREADS / 64; ++ w)
			x += red[w][tid];
		partial[(int64_t)chunk_slot[ch] * HUB_STRIDE + tid] = x;
	}
}

// stage 2: one wave per hub destination, lane k adds value k of its partials in ascending chunk order
__global__ __launch_bounds__(256)
void hub_final_kernel(int64_t n_hub, const int32_t *__restrict__ hub_dst, const int32_t *__restrict__ hub_kind,
	const int32_t *__restrict__ hub_slot_ptr, const int64_t *__restrict__ dst_off, const int64_t *__restrict__ dst_eoff,
	const int32_t *__restrict__ dst_flags, const double *__restrict__ partial, double damping, double *__restrict__ vals,
	double *__restrict__ eta)
{
	const int64_t h = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	const int k = threadIdx.x & 63;
	if(h >= n_hub)
		return;
	const int kind = hub_kind[h];
	const int nv = (kind == TernaryPlan::K02) ? 36 : (kind == TernaryPlan::K12) ? 18 : 27;
	if(k >= nv)
		return;
	const int32_t s0 = hub_slot_ptr[h], s1 = hub_slot_ptr[h + 1];
	double x = partial[(int64_t)s0 * HUB_STRIDE + k];
	for(int32_t sl = s0 + 1; sl < s1; ++ sl)
		x += partial[(int64_t)sl * HUB_STRIDE + k];
	const int32_t d = hub_dst[h], flags = dst_flags[d];
	double *o = vals + dst_off[d], *eo = eta + dst_eoff[d];
	if(kind == TernaryPlan::K02)
		border_store_value<TernaryPlan::K02>(k, x, flags, damping, o, eo);
	else if(kind == TernaryPlan::K12)
		border_store_value<TernaryPlan::K12>(k, x, flags, damping, o, eo);
	else
		border_store_value<TernaryPlan::K22>(k, x, flags, damping, o, eo);
}

// launches: those of the binary plan + per kind one sequential and one stage-1 launch + one stage-2 launch
void assemble_ternary_run(spp_ctx *ctx, const double *J0, const double *J1, const double *J2, const double *Om, const double *r,
	double damping, double *vals, double *eta)
{
	AssemblePlan *ap = ctx->assemble;
	TernaryPlan *tp = ap->ternary;
	assemble_run(ctx, J0, J1, Om, r, damping, vals, eta);
	hipStream_t s = ctx->stream;
#define SPP_BORDER_LAUNCH(KIND) \
	if(tp->n_seq[KIND]) \
		hipLaunchKernelGGL((border_seq_kernel<KIND>), dim3((unsigned)((tp->n_seq[KIND] + 255) / 256)), dim3(256), 0, s, \
			tp->n_seq[KIND], tp->seq_list[KIND].p, tp->dst_ptr.p, tp->dst_edge.p, tp->dst_off.p, tp->dst_eoff.p, tp->dst_flags.p, \
			J0, J1, J2, Om, r, damping, vals, eta); \
	if(tp->n_chunk[KIND]) \
		hipLaunchKernelGGL((hub_chunk_kernel<KIND>), dim3((unsigned)tp->n_chunk[KIND]), dim3(HUB_THREADS), 0, s, \
			tp->chunk_dst[KIND].p, tp->chunk_beg[KIND].p, tp->chunk_slot[KIND].p, tp->dst_ptr.p, tp->dst_edge.p, \
			J0, J1, J2, Om, r, tp->partial.p);
	SPP_BORDER_LAUNCH(TernaryPlan::K02)
	SPP_BORDER_LAUNCH(TernaryPlan::K12)
	SPP_BORDER_LAUNCH(TernaryPlan::K22)
#undef SPP_BORDER_LAUNCH
	if(tp->n_hub)
		hipLaunchKernelGGL(hub_final_kernel, dim3((unsigned)((tp->n_hub + 3) / 4)), dim3(256), 0, s,
			tp->n_hub, tp->hub_dst.p, tp->hub_kind.p, tp->hub_slot_ptr.p, tp->dst_off.p, tp->dst_eoff.p, tp->dst_flags.p,
			tp->partial.p, damping, vals, eta);
	SPP_HIP_CHECK(hipGetLastError());
}

} // namespace spp
