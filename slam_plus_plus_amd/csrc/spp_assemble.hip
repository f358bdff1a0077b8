// spp_assemble.hip -- Lambda = J^T Omega J and eta = J^T Omega r on gfx950, fp64.
//
// Replaces
//   symbolic: CLambdaOps2::AddEntriesInSparseSystem + Alloc_HessianBlocks_v2
//             (reference include/slam/NonlinearSolver_Lambda_Base.h:1852-1931, include/slam/BaseTypes_Binary.h:525-660)
//   numeric : Refresh_Lambda = Calculate_Hessians_v2 over all edges + CMatrixReductionPlan::ReduceAll
//             + CVectorReductionPlan::ReduceAll (_Lambda_Base.h:1658-1688, BaseTypes_Binary.h:759-848,
//             _Lambda_Base.h:563-607,743-756,152-197,395-399), the unary factor (:1903-1924) and the
//             Levenberg-Marquardt damping (NonlinearSolver_Lambda_LM.h:228-239).
//
// The reference writes every edge's H00 / H11 / g0 / g1 into temporaries and then gather-sums them
// per destination (1.02 GB of temporaries per refresh on Venice). Here the reduction
// plan is kept (same destinations, same edge order) but nothing is materialized: each destination
// block recomputes its contributions straight from J / Omega / r, which are read three times
// (off-diagonal block, vertex 0, vertex 1) and Lambda is written once.
//   offdiag_kernel   one thread per off-diagonal block: sum over its edges of J0^T Omega J1 (or the
//                    transposed form when the vertex ids are reversed, BaseTypes_Binary.h:783-806)
//   vertex_seq_kernel one thread per low-degree vertex, contributions summed sequentially in edge order
//                    (bit-identical to the reference's order: first assigned, rest added)
//   vertex_wave_kernel one wave per high-degree vertex (cameras): lanes stride over the edge list,
//                    fixed butterfly reduction => reproducible, order differs from sequential in the
//                    last bits only
// All three are HBM-bound: 192 B read + 144 B written per BA observation for the off-diagonal part.
// The plan (AssemblePlan) and the per-edge bodies jt_omega / vertex_contrib live in spp_assemble_plan.h: spp_assemble3.hip
// (ternary edges) runs these kernels on its (camera, point) part and adds the kernels of what touches an intrinsics vertex.

#include "spp_assemble_plan.h"
#include <algorithm>
#include <cstdint>

namespace spp {

void assemble_release(spp_ctx *ctx)
{
	delete ctx->assemble;
	ctx->assemble = nullptr;
}

void assemble_get_structure(const spp_ctx *ctx, int64_t *col_ptr, int64_t *row_idx, int64_t *blk_off)
{
	const Structure &st = ctx->assemble->st;
	std::copy(st.col_ptr.begin(), st.col_ptr.end(), col_ptr);
	std::copy(st.row_idx.begin(), st.row_idx.end(), row_idx);
	std::copy(st.blk_off.begin(), st.blk_off.end(), blk_off);
}

void assemble_set_edge_weights(spp_ctx *ctx, int group, const double *d_w)
{
	// (7,3,2): the reference's "first vertex carries the weight twice" rule (BaseTypes_Binary.h:768-848) would attach to the
	// landmark there (its typelist is (XYZ, CamSim3), the library's order is camera first): refused rather than half right
	SPP_REQUIRE(!d_w || ctx->assemble->d0[group] != 7, SPP_E_UNSUPPORTED, "robust weights on (7,3,2) edges");
	ctx->assemble->edge_weights[group] = d_w;
}

bool assemble_is_ternary(const spp_ctx *ctx)
{
	return ctx->assemble->ternary != nullptr;
}

int assemble_n_groups(const spp_ctx *ctx)
{
	return ctx->assemble->n_groups;
}

int64_t assemble_group_edges(const spp_ctx *ctx, int group)
{
	return ctx->assemble->gstart[group + 1] - ctx->assemble->gstart[group];
}

bool assemble_group_is_unary(const spp_ctx *ctx, int group)
{
	return ctx->assemble->d1[group] == 0;
}

static bool same_shape(const AssemblePlan *ap, int ga, int gb)
{
	return ap->d0[ga] == ap->d0[gb] && ap->d1[ga] == ap->d1[gb] && ap->rd[ga] == ap->rd[gb];
}

static bool shape_instantiated(int d0, int d1, int rd)
{
	return (d0 == 6 && d1 == 3 && rd == 2) || (d0 == 3 && d1 == 3 && rd == 3) || (d0 == 6 && d1 == 6 && rd == 6) ||
		(d0 == 3 && d1 == 2 && rd == 2) || (d0 == 6 && d1 == 3 && rd == 3) || (d0 == 6 && d1 == 3 && rd == 1) ||
		(d0 == 7 && d1 == 3 && rd == 2);
}

// a group of unary edges (d1 = 0, no second vertex array): (d0, rd) = (3,3) landmark / 2D pose prior, (6,6) pose prior
static bool unary_shape_instantiated(int d0, int rd)
{
	return (d0 == 3 && rd == 3) || (d0 == 6 && rd == 6);
}

void assemble_analyze(spp_ctx *ctx, int64_t nv, const int32_t *dim, int n_groups, const int64_t *g_ne,
	const int64_t *const *g_v0, const int64_t *const *g_v1, const int64_t *const *g_seq, const int *g_d0, const int *g_d1,
	const int *g_rd, int64_t unary_vertex, const uint8_t *skip_vertex)
{
	assemble_release(ctx); // after a rejected call the ctx has NO assembly plan (spp_assemble_device then fails its state check)
	SPP_REQUIRE(n_groups >= 1 && n_groups <= SPP_MAX_EDGE_GROUPS, SPP_E_UNSUPPORTED, "more than SPP_MAX_EDGE_GROUPS edge groups");
	int64_t ne = 0;
	bool any_unary = false;
	for(int g = 0; g < n_groups; ++ g) {
		if(g_d1[g] == 0 && !g_v1[g]) { // unary edges on v0 (BaseTypes_Unary.h): no second vertex, no off-diagonal block
			SPP_REQUIRE(unary_shape_instantiated(g_d0[g], g_rd[g]), SPP_E_UNSUPPORTED,
				"unary edge group (d0, rd) not instantiated: (3,3) (6,6)");
			any_unary = true;
		} else {
			SPP_REQUIRE(shape_instantiated(g_d0[g], g_d1[g], g_rd[g]), SPP_E_UNSUPPORTED,
				"edge group (d0, d1, rd) not instantiated: (6,3,2) (3,3,3) (6,6,6) (3,2,2) (6,3,3) (6,3,1) (7,3,2)");
			// (7,3,2) (Sim(3) cameras) has bodies in the one-group kernels only: it is the one group of its plan
			SPP_REQUIRE(g_d0[g] != 7 || n_groups == 1, SPP_E_UNSUPPORTED, "a (7,3,2) edge group must be the only group of its plan");
		}
		ne += g_ne[g];
	}
	SPP_REQUIRE(ne < (int64_t(1) << 30), SPP_E_UNSUPPORTED, "too many edges for 31-bit edge indices");
	VClock clk("assemble_analyze");
	const int nt = plan_threads(ne);
	for(int g = 0; g < n_groups; ++ g) {
		const int64_t *v0 = g_v0[g], *v1 = g_v1[g], gne = g_ne[g];
		const int d0 = g_d0[g], d1 = g_d1[g];
		if(!v1) { // unary: one vertex, nothing to be equal to
			run_threads(nt, [&](int t) {
				for(int64_t e = gne * t / nt, e1 = gne * (t + 1) / nt; e < e1; ++ e) {
					SPP_REQUIRE(v0[e] >= 0 && v0[e] < nv, SPP_E_BADARG, "bad edge");
					SPP_REQUIRE(dim[v0[e]] == d0, SPP_E_BADARG, "vertex width does not match the edge group");
				}
			});
			continue;
		}
		run_threads(nt, [&](int t) {
			for(int64_t e = gne * t / nt, e1 = gne * (t + 1) / nt; e < e1; ++ e) {
				SPP_REQUIRE(v0[e] >= 0 && v0[e] < nv && v1[e] >= 0 && v1[e] < nv && v0[e] != v1[e], SPP_E_BADARG, "bad edge");
				SPP_REQUIRE(dim[v0[e]] == d0 && dim[v1[e]] == d1, SPP_E_BADARG, "vertex width does not match the edge group");
			}
		});
	}
	SPP_REQUIRE(unary_vertex < nv, SPP_E_BADARG, "unary_vertex out of range");
	// built in a local object, installed in the ctx only when complete
	struct PlanGuard { AssemblePlan *p; ~PlanGuard() { delete p; } } guard = {new AssemblePlan};
	AssemblePlan *ap = guard.p;
	ap->n_groups = n_groups; ap->nv = nv; ap->ne = ne; ap->unary_vertex = unary_vertex;
	for(int g = 0; g < n_groups; ++ g) {
		ap->d0[g] = g_d0[g]; ap->d1[g] = g_d1[g]; ap->rd[g] = g_rd[g];
		ap->gstart[g + 1] = ap->gstart[g] + g_ne[g];
		for(int w : {g_d0[g], g_d1[g]}) {
			if(w && std::find(ap->cls_dim, ap->cls_dim + ap->n_cls, w) == ap->cls_dim + ap->n_cls)
				ap->cls_dim[ap->n_cls ++] = w;
		}
		int s = 0; // a shape is (d0, d1, rd): (6,3,2) and (6,3,3) share their widths
		while(s < ap->n_shapes && !same_shape(ap, ap->shape_group[s], g))
			++ s;
		if(s == ap->n_shapes)
			ap->shape_group[ap->n_shapes ++] = g;
	}
	// two shapes of the same widths could feed ONE off-diagonal block (a pose-landmark pair joined by a (6,3,2) and by a
	// (6,3,3) edge), which no off-diagonal kernel sums: such a plan is rejected as a whole
	for(int a = 0; a < ap->n_shapes; ++ a) {
		for(int b = a + 1; b < ap->n_shapes; ++ b) {
			const int ga = ap->shape_group[a], gb = ap->shape_group[b];
			SPP_REQUIRE(ap->d0[ga] != ap->d0[gb] || ap->d1[ga] != ap->d1[gb], SPP_E_UNSUPPORTED,
				"two of the edge groups (6,3,1), (6,3,2), (6,3,3) in one plan: their off-diagonal blocks could mix two shapes");
		}
	}
	// ---- the edges in the order of their global positions: everything below walks positions, v0[q] / v1[q] are the vertices
	// of the edge at position q and edge_at(q) its index in the concatenation of the groups. One group without h_seq: the
	// caller's arrays as they stand
	const int64_t *v0 = g_v0[0], *v1 = g_v1[0];
	HVec<int64_t> pv0, pv1;
	HVec<int32_t> pedge;
	const bool identity = n_groups == 1 && !(g_seq && g_seq[0]) && !any_unary;
	if(!identity) {
		pv0.resize(ne);
		pv1.resize(ne);
		pedge.assign(ne, -1);
		for(int g = 0; g < n_groups; ++ g) {
			const int64_t *seq = g_seq ? g_seq[g] : nullptr;
			for(int64_t e = 0; e < g_ne[g]; ++ e) {
				const int64_t q = seq ? seq[e] : ap->gstart[g] + e;
				SPP_REQUIRE(q >= 0 && q < ne && pedge[q] < 0, SPP_E_BADARG, "h_seq is not a permutation of the edge positions");
				pedge[q] = (int32_t)(ap->gstart[g] + e);
				pv0[q] = g_v0[g][e];
				pv1[q] = g_v1[g] ? g_v1[g][e] : -1; // unary: no second vertex
			}
		}
		v0 = pv0.data();
		v1 = pv1.data();
	}
	auto edge_at = [&](int64_t q) { return identity ? (int32_t)q : pedge[q]; };
	// ---- Lambda structure: diagonal of every vertex + upper block of every edge
	// (_Lambda_Base.h:1863-1881 builds all block rows/cols first, then :1897 allocates edge blocks)
	HVec<std::pair<int64_t, int64_t> > key(ne); // (col, row)
	run_threads(nt, [&](int t) {
		for(int64_t e = ne * t / nt, e1 = ne * (t + 1) / nt; e < e1; ++ e)
			key[e] = v1[e] < 0 ? std::make_pair(nv, v0[e]) : std::make_pair(std::max(v0[e], v1[e]), std::min(v0[e], v1[e]));
	});
	// (a unary edge has no block: it is filed under a column past the last, which the loops over the columns never visit)
	// edges in (column, row, edge index) order: a counting sort by column, then (row, edge) inside each column -- a handful
	// per landmark column -- by insertion, longer runs by std::sort (a comparison sort of all the edges was most of this
	// function on a Venice-sized graph)
	HVec<int64_t> eorder(ne);
	std::vector<int64_t> cstart(nv + 1 + (any_unary ? 1 : 0), 0); // edges of column c: eorder[cstart[c] .. cstart[c + 1])
	std::vector<int64_t> ccut; // ranges of columns with about equal numbers of edges (+ 1 per column)
	{
		// counted and scattered by all threads with atomic increments; the scatter is then in no particular order, the sort
		// inside each column is by (row, edge index) and restores it
		run_threads(nt, [&](int t) {
			for(int64_t e = ne * t / nt, e1 = ne * (t + 1) / nt; e < e1; ++ e)
				__atomic_fetch_add(&cstart[key[e].first + 1], (int64_t)1, __ATOMIC_RELAXED);
		});
		for(int64_t c = 0; c < nv; ++ c)
			cstart[c + 1] += cstart[c];
		std::vector<int64_t> fill(cstart.begin(), cstart.end() - 1);
		run_threads(nt, [&](int t) {
			for(int64_t e = ne * t / nt, e1 = ne * (t + 1) / nt; e < e1; ++ e)
				eorder[__atomic_fetch_add(&fill[key[e].first], (int64_t)1, __ATOMIC_RELAXED)] = e;
		});
		{
			std::vector<int64_t> w(nv + 1);
			for(int64_t c = 0; c <= nv; ++ c)
				w[c] = cstart[c] + c;
			balanced_cuts(w, nt, ccut);
		}
		run_threads(nt, [&](int t) {
		for(int64_t c = ccut[t]; c < ccut[t + 1]; ++ c) {
			const int64_t b = cstart[c], n = cstart[c + 1] - b;
			if(n <= 1)
				continue;
			if(n > 32) {
				std::sort(eorder.begin() + b, eorder.begin() + b + n, [&](int64_t x, int64_t y) {
					return key[x].second != key[y].second ? key[x].second < key[y].second : x < y; });
				continue;
			}
			for(int64_t i = 1; i < n; ++ i) { // insertion sort by (row, edge)
				const int64_t x = eorder[b + i], rx = key[x].second;
				int64_t j = i;
				for(; j > 0; -- j) {
					const int64_t y = eorder[b + j - 1], ry = key[y].second;
					if(ry < rx || (ry == rx && y < x))
						break;
					eorder[b + j] = y;
				}
				eorder[b + j] = x;
			}
		}
		});
	}
	clk.lap("edges sorted by block");
	Structure &st = ap->st;
	st.nb = nv;
	st.dim.assign(dim, dim + nv);
	st.base.resize(nv + 1);
	st.base[0] = 0;
	for(int64_t v = 0; v < nv; ++ v)
		st.base[v + 1] = st.base[v] + dim[v];
	st.n = st.base[nv];
	// Columns are independent once the edges are in block order: a first pass counts the blocks and values of every column
	// (ranges of columns on host threads), a serial prefix gives every column its place, a second pass writes.
	st.col_ptr.assign(nv + 1, 0);
	HVec<int64_t> v_doff(nv), c_ob(nv + 1, 0), c_off(nv + 1, 0); // per column: first off-diagonal block, first value
	run_threads(nt, [&](int t) {
		for(int64_t c = ccut[t]; c < ccut[t + 1]; ++ c) {
			int64_t nblk = 0, nval = 0, rprev = -1;
			for(int64_t q = cstart[c]; q < cstart[c + 1]; ++ q) {
				const int64_t r = key[eorder[q]].second;
				if(r != rprev) {
					++ nblk;
					nval += (int64_t)dim[r] * dim[c];
					rprev = r;
				}
			}
			c_ob[c + 1] = nblk;
			c_off[c + 1] = nval + (int64_t)dim[c] * dim[c];
		}
	});
	for(int64_t c = 0; c < nv; ++ c) {
		st.col_ptr[c + 1] = st.col_ptr[c] + c_ob[c + 1] + 1;
		c_ob[c + 1] += c_ob[c];
		c_off[c + 1] += c_off[c];
	}
	st.nnzb = st.col_ptr[nv];
	st.nvals = c_off[nv];
	const int64_t n_ob = c_ob[nv];
	HVec<int32_t> ob_ptr(n_ob + 1), ob_edge(ne);
	HVec<int64_t> ob_off(n_ob);
	ob_ptr[0] = 0;
	st.row_idx.resize(st.nnzb);
	st.blk_off.resize(st.nnzb);
	run_threads(nt, [&](int t) {
		for(int64_t c = ccut[t]; c < ccut[t + 1]; ++ c) {
			int64_t p = st.col_ptr[c], k = c_ob[c], off = c_off[c], q = cstart[c];
			const int64_t qe = cstart[c + 1];
			while(q < qe) {
				const int64_t r = key[eorder[q]].second;
				st.row_idx[p] = r;
				st.blk_off[p] = off;
				++ p;
				ob_off[k] = off;
				off += (int64_t)dim[r] * dim[c];
				for(; q < qe && key[eorder[q]].second == r; ++ q) {
					const int64_t e = eorder[q]; // stable sort: edges of one block stay in the order of their positions
					ob_edge[q] = edge_at(e) | (v0[e] > v1[e] ? (int32_t)0x80000000 : 0);
				}
				ob_ptr[++ k] = (int32_t)q;
			}
			st.row_idx[p] = c;
			st.blk_off[p] = off;
			v_doff[c] = off;
		}
	});
	ap->n_ob = (int64_t)ob_off.size();
	clk.lap("Lambda structure");
	// ---- per-vertex contribution lists in edge order: (edge, side)
	HVec<int32_t> vl_ptr(nv + 1, 0), vl_entry(2 * ne);
	// (serial: the camera side of a BA graph is a few hundred counters that every edge increments -- atomic increments from
	// 16 threads on them measured 125 ms against 7 ms for this loop)
	for(int64_t e = 0; e < ne; ++ e) {
		++ vl_ptr[v0[e] + 1];
		if(v1[e] >= 0)
			++ vl_ptr[v1[e] + 1];
	}
	for(int64_t v = 0; v < nv; ++ v)
		vl_ptr[v + 1] += vl_ptr[v];
	{
		HVec<int32_t> fill(vl_ptr.begin(), vl_ptr.end() - 1);
		for(int64_t e = 0; e < ne; ++ e) { // within an edge vertex 0 registers before vertex 1
			vl_entry[fill[v0[e]] ++] = edge_at(e) << 1;
			if(v1[e] >= 0)
				vl_entry[fill[v1[e]] ++] = (edge_at(e) << 1) | 1;
		}
	}
	std::vector<int32_t> lseq[MAX_WIDTH_CLASSES], lwave[MAX_WIDTH_CLASSES];
	for(int64_t v = 0; v < nv; ++ v) {
		const int cls = (int)(std::find(ap->cls_dim, ap->cls_dim + ap->n_cls, dim[v]) - ap->cls_dim);
		SPP_REQUIRE(cls < ap->n_cls, SPP_E_BADARG, "vertex width outside of the edge group");
		if(skip_vertex && skip_vertex[v])
			continue; // in no list: another kernel writes its diagonal block and eta segment (spp_assemble3.hip)
		if(vl_ptr[v + 1] - vl_ptr[v] <= SEQ_MAX_DEGREE)
			lseq[cls].push_back((int32_t)v);
		else
			lwave[cls].push_back((int32_t)v);
	}
	// several shapes: the off-diagonal blocks of each (a block's edges share its two widths, hence its shape: the one pair of shapes with equal widths was rejected above); one launch each
	std::vector<int32_t> loblist[SPP_MAX_EDGE_GROUPS];
	if(ap->n_shapes > 1) {
		for(int64_t b = 0; b < n_ob; ++ b) {
			const int32_t e = ob_edge[ob_ptr[b]] & 0x7fffffff;
			int g = 0;
			while(e >= ap->gstart[g + 1])
				++ g;
			int sh = 0;
			while(!same_shape(ap, ap->shape_group[sh], g))
				++ sh;
			loblist[sh].push_back((int32_t)b);
		}
	}
	clk.lap("vertex lists");
	hipStream_t s = ctx->stream;
	UploadArena arena(s);
	arena.add(ap->ob_ptr, ob_ptr);
	arena.add(ap->ob_edge, ob_edge);
	arena.add(ap->ob_off, ob_off);
	arena.add(ap->vl_ptr, vl_ptr);
	arena.add(ap->vl_entry, vl_entry);
	arena.add(ap->v_doff, v_doff);
	{
		std::vector<int64_t> vb(st.base.begin(), st.base.end() - 1);
		arena.add(ap->v_base, vb);
	}
	for(int sh = 0; sh < ap->n_shapes && ap->n_shapes > 1; ++ sh) {
		ap->n_oblist[sh] = (int64_t)loblist[sh].size();
		arena.add(ap->oblist[sh], loblist[sh]);
	}
	for(int cls = 0; cls < ap->n_cls; ++ cls) {
		ap->n_seq[cls] = (int64_t)lseq[cls].size();
		ap->n_wave[cls] = (int64_t)lwave[cls].size();
		arena.add(ap->vlist_seq[cls], lseq[cls]);
		arena.add(ap->vlist_wave[cls], lwave[cls]);
	}
	arena.commit(ap->index_store);
	SPP_HIP_CHECK(hipStreamSynchronize(s));
	clk.lap("uploads");
	// complete: install. The ctx now describes this Lambda (sizes for spp_get_info before spp_analyze is called);
	// a solve plan analyzed for a DIFFERENT structure is dropped rather than left beside the new sizes
	if(ctx->mode >= 0 && (ctx->st.nb != st.nb || ctx->st.n != st.n || ctx->st.nnzb != st.nnzb || ctx->st.nvals != st.nvals))
		ctx->mode = -1;
	ctx->st.nb = st.nb; ctx->st.n = st.n; ctx->st.nnzb = st.nnzb; ctx->st.nvals = st.nvals;
	ctx->assemble = ap;
	guard.p = nullptr;
}

// --------------------------------------------------------------------------------------------------
// device helpers
// --------------------------------------------------------------------------------------------------
template <int D0, int D1, int RD>
__global__ __launch_bounds__(256)
void offdiag_kernel(int64_t n_ob, const int32_t *__restrict__ ob_ptr, const int32_t *__restrict__ ob_edge,
	const int64_t *__restrict__ ob_off, const double *__restrict__ J0, const double *__restrict__ J1,
	const double *__restrict__ Om, const double *__restrict__ wts, double *__restrict__ vals)
{
	const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(b >= n_ob)
		return;
	double acc[D0 * D1];
	bool first = true;
	for(int32_t q = ob_ptr[b]; q < ob_ptr[b + 1]; ++ q) {
		const int32_t ee = ob_edge[q];
		const int64_t e = ee & 0x7fffffff;
		const bool rev = ee < 0;
		double j0[RD * D0], j1[RD * D1], om[RD * RD], T[D0 * RD];
#pragma unroll
		for(int i = 0; i < RD * D0; ++ i) j0[i] = J0[e * RD * D0 + i];
#pragma unroll
		for(int i = 0; i < RD * D1; ++ i) j1[i] = J1[e * RD * D1 + i];
#pragma unroll
		for(int i = 0; i < RD * RD; ++ i) om[i] = Om[e * RD * RD + i];
		jt_omega<D0, RD>(j0, om, T);
		if(wts) { // robust edge: t_H0_sigma_inv = J0^T Sigma^-1 w (BaseTypes_Binary.h:771)
			const double wgt = wts[e];
#pragma unroll
			for(int i = 0; i < D0 * RD; ++ i)
				T[i] *= wgt;
		}
		// H01 (D0 x D1) = T J1 ; stored as is, or transposed (D1 x D0) when the ids are reversed
#pragma unroll
		for(int c = 0; c < D1; ++ c)
#pragma unroll
			for(int i = 0; i < D0; ++ i) {
				double s = 0;
#pragma unroll
				for(int l = 0; l < RD; ++ l)
					s += T[i + l * D0] * j1[l + c * RD];
				const int idx = rev ? (c + i * D1) : (i + c * D0);
				acc[idx] = first ? s : acc[idx] + s;
			}
		first = false;
	}
	double *o = vals + ob_off[b];
#pragma unroll
	for(int i = 0; i < D0 * D1; ++ i)
		o[i] = acc[i];
}

// D = width of the vertices handled; when D0 == D1 a vertex may sit on either side of its edges
template <int D, int D0, int D1, int RD>
__device__ __forceinline__ void load_contrib(int32_t entry, const double *__restrict__ J0, const double *__restrict__ J1,
	const double *__restrict__ Om, const double *__restrict__ r, const double *__restrict__ wts, double *H, double *g)
{
	const int64_t e = entry >> 1;
	const int side = entry & 1;
	const double wgt = wts ? wts[e] : 1.0;
	double om[RD * RD], rr[RD], j[RD * D];
#pragma unroll
	for(int i = 0; i < RD * RD; ++ i) om[i] = Om[e * RD * RD + i];
#pragma unroll
	for(int i = 0; i < RD; ++ i) rr[i] = r[e * RD + i];
	if(side == 0) {
		if(D == D0) {
#pragma unroll
			for(int i = 0; i < RD * D; ++ i) j[i] = J0[e * RD * D0 + i];
			vertex_contrib<D, RD, 0>(j, om, rr, wgt, H, g);
		}
	} else {
		if(D == D1) {
#pragma unroll
			for(int i = 0; i < RD * D; ++ i) j[i] = J1[e * RD * D1 + i];
			vertex_contrib<D, RD, 1>(j, om, rr, wgt, H, g);
		}
	}
}

// a unary edge's contribution to its one vertex (Calculate_Hessians_v2, BaseTypes_Unary.h:547-587): H00 = J0^T Omega J0 w,
// g0 = J0^T (Omega r w) -- the robust weight ONCE on each, where the reference applies it (:560-569; 1 for a plain edge)
template <int D, int RD>
__device__ __forceinline__ void load_unary(int64_t e, const double *__restrict__ J0, const double *__restrict__ Om,
	const double *__restrict__ r, const double *__restrict__ wts, double *H, double *g)
{
	const double wgt = wts ? wts[e] : 1.0;
	double om[RD * RD], j[RD * D], T[D * RD], orr[RD];
#pragma unroll
	for(int i = 0; i < RD * RD; ++ i) om[i] = Om[e * RD * RD + i];
#pragma unroll
	for(int i = 0; i < RD * D; ++ i) j[i] = J0[e * RD * D + i];
	jt_omega<D, RD>(j, om, T);
#pragma unroll
	for(int c = 0; c < D; ++ c)
#pragma unroll
		for(int i = 0; i <= c; ++ i) {
			double s = 0;
#pragma unroll
			for(int l = 0; l < RD; ++ l)
				s += T[i + l * D] * j[l + c * RD];
			H[i + c * D] = s * wgt;
		}
#pragma unroll
	for(int l = 0; l < RD; ++ l) {
		double s = 0;
#pragma unroll
		for(int m = 0; m < RD; ++ m)
			s += om[l + m * RD] * r[e * RD + m];
		orr[l] = s * wgt;
	}
#pragma unroll
	for(int i = 0; i < D; ++ i) {
		double s = 0;
#pragma unroll
		for(int l = 0; l < RD; ++ l)
			s += j[l + i * RD] * orr[l];
		g[i] = s;
	}
}

template <int D>
__device__ __forceinline__ void store_vertex(const double *H, const double *g, bool unary, double damping,
	double *__restrict__ hd, double *__restrict__ gd)
{
#pragma unroll
	for(int c = 0; c < D; ++ c)
#pragma unroll
		for(int i = 0; i <= c; ++ i) {
			double v = H[i + c * D];
			if(i == c) {
				if(unary)
					v += 1.0;  // UF^T UF = identity, last in the reduction list (_Lambda_Base.h:1903-1924)
				v += damping;   // Lambda_ii.diagonal() += alpha (NonlinearSolver_Lambda_LM.h:228-239)
			}
			hd[i + c * D] = v;
			hd[c + i * D] = v;  // selfadjointView<Upper>: lower half mirrors the upper
		}
#pragma unroll
	for(int i = 0; i < D; ++ i)
		gd[i] = g[i];
}

template <int D, int D0, int D1, int RD>
__global__ __launch_bounds__(256)
void vertex_seq_kernel(int64_t nlist, const int32_t *__restrict__ vlist, const int32_t *__restrict__ vl_ptr,
	const int32_t *__restrict__ vl_entry, const int64_t *__restrict__ v_doff, const int64_t *__restrict__ v_base,
	const double *__restrict__ J0, const double *__restrict__ J1, const double *__restrict__ Om,
	const double *__restrict__ r, const double *__restrict__ wts, int64_t unary_vertex, double damping, double *__restrict__ vals,
	double *__restrict__ eta)
{
	const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(t >= nlist)
		return;
	const int32_t v = vlist[t];
	double H[D * D], g[D];
#pragma unroll
	for(int i = 0; i < D * D; ++ i) H[i] = 0;
#pragma unroll
	for(int i = 0; i < D; ++ i) g[i] = 0;
	bool first = true;
	for(int32_t q = vl_ptr[v]; q < vl_ptr[v + 1]; ++ q) {
		double Hc[D * D], gc[D];
		load_contrib<D, D0, D1, RD>(vl_entry[q], J0, J1, Om, r, wts, Hc, gc);
		if(first) { // the first source is assigned, the others are added (_Lambda_Base.h:598-604)
#pragma unroll
			for(int c = 0; c < D; ++ c)
#pragma unroll
				for(int i = 0; i <= c; ++ i) H[i + c * D] = Hc[i + c * D];
#pragma unroll
			for(int i = 0; i < D; ++ i) g[i] = gc[i];
			first = false;
		} else {
#pragma unroll
			for(int c = 0; c < D; ++ c)
#pragma unroll
				for(int i = 0; i <= c; ++ i) H[i + c * D] += Hc[i + c * D];
#pragma unroll
			for(int i = 0; i < D; ++ i) g[i] += gc[i];
		}
	}
	store_vertex<D>(H, g, v == unary_vertex, damping, vals + v_doff[v], eta + v_base[v]);
}

template <int D, int D0, int D1, int RD>
__global__ __launch_bounds__(256)
void vertex_wave_kernel(int64_t nlist, const int32_t *__restrict__ vlist, const int32_t *__restrict__ vl_ptr,
	const int32_t *__restrict__ vl_entry, const int64_t *__restrict__ v_doff, const int64_t *__restrict__ v_base,
	const double *__restrict__ J0, const double *__restrict__ J1, const double *__restrict__ Om,
	const double *__restrict__ r, const double *__restrict__ wts, int64_t unary_vertex, double damping, double *__restrict__ vals,
	double *__restrict__ eta)
{
	const int64_t t = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	const int lane = threadIdx.x & 63;
	if(t >= nlist)
		return;
	const int32_t v = vlist[t];
	double H[D * D], g[D];
#pragma unroll
	for(int i = 0; i < D * D; ++ i) H[i] = 0;
#pragma unroll
	for(int i = 0; i < D; ++ i) g[i] = 0;
	for(int32_t q = vl_ptr[v] + lane; q < vl_ptr[v + 1]; q += 64) {
		double Hc[D * D], gc[D];
		load_contrib<D, D0, D1, RD>(vl_entry[q], J0, J1, Om, r, wts, Hc, gc);
#pragma unroll
		for(int c = 0; c < D; ++ c)
#pragma unroll
			for(int i = 0; i <= c; ++ i) H[i + c * D] += Hc[i + c * D];
#pragma unroll
		for(int i = 0; i < D; ++ i) g[i] += gc[i];
	}
#pragma unroll
	for(int c = 0; c < D; ++ c)
#pragma unroll
		for(int i = 0; i <= c; ++ i) {
			double x = H[i + c * D];
#pragma unroll
			for(int off = 32; off > 0; off >>= 1)
				x += __shfl_xor(x, off);
			H[i + c * D] = x;
		}
#pragma unroll
	for(int i = 0; i < D; ++ i) {
		double x = g[i];
#pragma unroll
		for(int off = 32; off > 0; off >>= 1)
			x += __shfl_xor(x, off);
		g[i] = x;
	}
	if(lane == 0)
		store_vertex<D>(H, g, v == unary_vertex, damping, vals + v_doff[v], eta + v_base[v]);
}

// --------------------------------------------------------------------------------------------------
// several edge groups (spp_assemble_groups_device): the same three kernels, with the pointer set of every group passed by
// value. A list entry is an index into the concatenation of the groups; comparing it with the (at most four) group starts
// gives the group, the group gives the pointers and the shape, and the shape selects the body instantiated for it. Every
// body is the one the one-group kernels run (jt_omega / vertex_contrib / load_contrib above), applied in the order of the
// lists: plain edges give the one-group kernels' bits (one shape split into two groups is bit-identical to the one group).
// With robust weights the compiler contracts w * s + sum into an FMA in some of the kernels and not in others, so weighted
// sums may differ from the one-group kernels' in the last bit; a plan of ONE group therefore runs the one-group kernels
// (assemble_groups_run), and the two entry points agree bit for bit on it whatever the weights. Traffic is unchanged: each edge's J / Omega / r is read by
// the three destinations it feeds; what the groups share is the launches.
// A group of UNARY edges (d1 = 0, no second vertex array: priors, reference include/slam/BaseTypes_Unary.h:547-587) feeds
// ONE destination, its vertex: an entry of side 0 in that vertex's list at the edge's position, no off-diagonal block
// (assemble_analyze files it under a column past the last), the body load_unary; its J1 pointer is never read.
// --------------------------------------------------------------------------------------------------
enum { SHAPE_632 = 0, SHAPE_333 = 1, SHAPE_666 = 2, SHAPE_322 = 3, SHAPE_633 = 4, SHAPE_631 = 5, SHAPE_U33 = 6, SHAPE_U66 = 7,
	SHAPE_732 = 8 /* one-group plans only: no body in the groups kernels */ };

struct GroupPtrs {
	const double *J0, *J1, *Om, *r, *w;
	int32_t start; // first index of the group in the concatenation; INT32_MAX past the last group
	int32_t shape;
};

struct GroupArgs { // (four members, not an array: every access is then a kernel argument in scalar registers, never scratch)
	GroupPtrs g0, g1, g2, g3;
};

// the operands of one edge: its group's arrays and its index inside them
struct EdgeRef {
	const double *J0, *J1, *Om, *r, *w;
	int32_t e, shape;
};

// (by value: `g == 0 ? ga.g0.m : ...` on the members themselves is a choice between ADDRESSES, which sends the argument
// struct to scratch)
template <class T>
__device__ __forceinline__ T pick4(int g, T a, T b, T c, T d)
{
	return g == 0 ? a : g == 1 ? b : g == 2 ? c : d;
}

__device__ __forceinline__ EdgeRef edge_ref(const GroupArgs &ga, int32_t ce)
{
	static_assert(SPP_MAX_EDGE_GROUPS == 4, "GroupArgs holds four groups");
	const int g = (ce >= ga.g1.start) + (ce >= ga.g2.start) + (ce >= ga.g3.start);
#define SPP_PICK(m) pick4(g, ga.g0.m, ga.g1.m, ga.g2.m, ga.g3.m)
	EdgeRef x;
	x.J0 = SPP_PICK(J0); x.J1 = SPP_PICK(J1); x.Om = SPP_PICK(Om); x.r = SPP_PICK(r); x.w = SPP_PICK(w);
	x.e = ce - SPP_PICK(start);
	x.shape = SPP_PICK(shape);
#undef SPP_PICK
	return x;
}

// the blocks oblist[0 .. n) (all blocks 0 .. n when null) have the shape (D0, D1, RD); their edges may come from any group of it
template <int D0, int D1, int RD>
__global__ __launch_bounds__(256)
void offdiag_groups_kernel(int64_t n, const int32_t *__restrict__ oblist, const int32_t *__restrict__ ob_ptr,
	const int32_t *__restrict__ ob_edge, const int64_t *__restrict__ ob_off, const GroupArgs ga, double *__restrict__ vals)
{
	const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(t >= n)
		return;
	const int64_t b = oblist ? oblist[t] : t;
	double acc[D0 * D1];
	bool first = true;
	for(int32_t q = ob_ptr[b]; q < ob_ptr[b + 1]; ++ q) {
		const int32_t ee = ob_edge[q];
		const EdgeRef x = edge_ref(ga, ee & 0x7fffffff);
		const int64_t e = x.e;
		const bool rev = ee < 0;
		double j0[RD * D0], j1[RD * D1], om[RD * RD], T[D0 * RD];
#pragma unroll
		for(int i = 0; i < RD * D0; ++ i) j0[i] = x.J0[e * RD * D0 + i];
#pragma unroll
		for(int i = 0; i < RD * D1; ++ i) j1[i] = x.J1[e * RD * D1 + i];
#pragma unroll
		for(int i = 0; i < RD * RD; ++ i) om[i] = x.Om[e * RD * RD + i];
		jt_omega<D0, RD>(j0, om, T);
		if(x.w) { // robust edge, as in offdiag_kernel
			const double wgt = x.w[e];
#pragma unroll
			for(int i = 0; i < D0 * RD; ++ i)
				T[i] *= wgt;
		}
#pragma unroll
		for(int c = 0; c < D1; ++ c)
#pragma unroll
			for(int i = 0; i < D0; ++ i) {
				double s = 0;
#pragma unroll
				for(int l = 0; l < RD; ++ l)
					s += T[i + l * D0] * j1[l + c * RD];
				const int idx = rev ? (c + i * D1) : (i + c * D0);
				acc[idx] = first ? s : acc[idx] + s;
			}
		first = false;
	}
	double *o = vals + ob_off[b];
#pragma unroll
	for(int i = 0; i < D0 * D1; ++ i)
		o[i] = acc[i];
}

// contribution of one list entry to a vertex of width D: the body of the entry's shape (a shape without a D-wide side
// cannot occur in the list of such a vertex). W633: the plan holds a (6,3,3) group; without one the switch is the four-way
// switch the kernels had before that shape existed, instruction for instruction (measured: with the fifth case compiled
// in, the 2D odometry + observation assembly of tools/slam2d_time.py took 46.7 us instead of 45.9 us). WEXT, likewise: the
// plan holds a (6,3,1) group or a group of unary edges (W633 is then set, too); without one the switch is the one above
template <int D, bool W633, bool WEXT>
__device__ __forceinline__ void load_contrib_groups(int32_t entry, const GroupArgs &ga, double *H, double *g)
{
	const EdgeRef x = edge_ref(ga, entry >> 1);
	const int32_t le = (x.e << 1) | (entry & 1);
	switch(x.shape) {
	case SHAPE_632:
		if(D == 6 || D == 3)
			load_contrib<D, 6, 3, 2>(le, x.J0, x.J1, x.Om, x.r, x.w, H, g);
		break;
	case SHAPE_333:
		if(D == 3)
			load_contrib<D, 3, 3, 3>(le, x.J0, x.J1, x.Om, x.r, x.w, H, g);
		break;
	case SHAPE_666:
		if(D == 6)
			load_contrib<D, 6, 6, 6>(le, x.J0, x.J1, x.Om, x.r, x.w, H, g);
		break;
	default:
		if(WEXT && x.shape >= SHAPE_631) {
			if(x.shape == SHAPE_631) {
				if(D == 6 || D == 3)
					load_contrib<D, 6, 3, 1>(le, x.J0, x.J1, x.Om, x.r, x.w, H, g);
			} else if(x.shape == SHAPE_U33) {
				if(D == 3)
					load_unary<3, 3>(x.e, x.J0, x.Om, x.r, x.w, H, g);
			} else if(D == 6)
				load_unary<6, 6>(x.e, x.J0, x.Om, x.r, x.w, H, g);
		} else if(W633 && x.shape == SHAPE_633) {
			if(D == 6 || D == 3)
				load_contrib<D, 6, 3, 3>(le, x.J0, x.J1, x.Om, x.r, x.w, H, g);
		} else if(D == 3 || D == 2)
			load_contrib<D, 3, 2, 2>(le, x.J0, x.J1, x.Om, x.r, x.w, H, g);
		break;
	}
}

template <int D, bool W633, bool WEXT = false>
__global__ __launch_bounds__(256)
void vertex_seq_groups_kernel(int64_t nlist, const int32_t *__restrict__ vlist, const int32_t *__restrict__ vl_ptr,
	const int32_t *__restrict__ vl_entry, const int64_t *__restrict__ v_doff, const int64_t *__restrict__ v_base,
	const GroupArgs ga, int64_t unary_vertex, double damping, double *__restrict__ vals, double *__restrict__ eta)
{
	const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(t >= nlist)
		return;
	const int32_t v = vlist[t];
	double H[D * D], g[D];
#pragma unroll
	for(int i = 0; i < D * D; ++ i) H[i] = 0;
#pragma unroll
	for(int i = 0; i < D; ++ i) g[i] = 0;
	bool first = true;
	for(int32_t q = vl_ptr[v]; q < vl_ptr[v + 1]; ++ q) {
		double Hc[D * D], gc[D];
		load_contrib_groups<D, W633, WEXT>(vl_entry[q], ga, Hc, gc);
		if(first) { // the first source is assigned, the others are added (_Lambda_Base.h:598-604)
#pragma unroll
			for(int c = 0; c < D; ++ c)
#pragma unroll
				for(int i = 0; i <= c; ++ i) H[i + c * D] = Hc[i + c * D];
#pragma unroll
			for(int i = 0; i < D; ++ i) g[i] = gc[i];
			first = false;
		} else {
#pragma unroll
			for(int c = 0; c < D; ++ c)
#pragma unroll
				for(int i = 0; i <= c; ++ i) H[i + c * D] += Hc[i + c * D];
#pragma unroll
			for(int i = 0; i < D; ++ i) g[i] += gc[i];
		}
	}
	store_vertex<D>(H, g, v == unary_vertex, damping, vals + v_doff[v], eta + v_base[v]);
}

template <int D, bool W633, bool WEXT = false>
__global__ __launch_bounds__(256)
void vertex_wave_groups_kernel(int64_t nlist, const int32_t *__restrict__ vlist, const int32_t *__restrict__ vl_ptr,
	const int32_t *__restrict__ vl_entry, const int64_t *__restrict__ v_doff, const int64_t *__restrict__ v_base,
	const GroupArgs ga, int64_t unary_vertex, double damping, double *__restrict__ vals, double *__restrict__ eta)
{
	const int64_t t = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	const int lane = threadIdx.x & 63;
	if(t >= nlist)
		return;
	const int32_t v = vlist[t];
	double H[D * D], g[D];
#pragma unroll
	for(int i = 0; i < D * D; ++ i) H[i] = 0;
#pragma unroll
	for(int i = 0; i < D; ++ i) g[i] = 0;
	for(int32_t q = vl_ptr[v] + lane; q < vl_ptr[v + 1]; q += 64) {
		double Hc[D * D], gc[D];
		load_contrib_groups<D, W633, WEXT>(vl_entry[q], ga, Hc, gc);
#pragma unroll
		for(int c = 0; c < D; ++ c)
#pragma unroll
			for(int i = 0; i <= c; ++ i) H[i + c * D] += Hc[i + c * D];
#pragma unroll
		for(int i = 0; i < D; ++ i) g[i] += gc[i];
	}
#pragma unroll
	for(int c = 0; c < D; ++ c)
#pragma unroll
		for(int i = 0; i <= c; ++ i) {
			double x = H[i + c * D];
#pragma unroll
			for(int off = 32; off > 0; off >>= 1)
				x += __shfl_xor(x, off);
			H[i + c * D] = x;
		}
#pragma unroll
	for(int i = 0; i < D; ++ i) {
		double x = g[i];
#pragma unroll
		for(int off = 32; off > 0; off >>= 1)
			x += __shfl_xor(x, off);
		g[i] = x;
	}
	if(lane == 0)
		store_vertex<D>(H, g, v == unary_vertex, damping, vals + v_doff[v], eta + v_base[v]);
}

static int shape_id(int d0, int d1, int rd)
{
	if(d1 == 0)
		return d0 == 6 ? SHAPE_U66 : SHAPE_U33;
	if(d0 == 7)
		return SHAPE_732;
	if(d0 == 6)
		return d1 == 6 ? SHAPE_666 : (rd == 3 ? SHAPE_633 : rd == 1 ? SHAPE_631 : SHAPE_632);
	return d1 == 3 ? SHAPE_333 : SHAPE_322;
}

// launches: one per distinct shape (off-diagonal blocks) + at most two per vertex width class -- whatever the graph's size
void assemble_groups_run(spp_ctx *ctx, const double *const *J0, const double *const *J1, const double *const *Om,
	const double *const *r, double damping, double *vals, double *eta)
{
	AssemblePlan *ap = ctx->assemble;
	if(ap->n_groups == 1 && ap->d1[0]) { // the one-group case IS spp_assemble_device: same kernels, same bits
		assemble_run(ctx, J0[0], J1[0], Om[0], r[0], damping, vals, eta);
		return;
	}
	hipStream_t s = ctx->stream;
	GroupArgs ga;
	GroupPtrs *gp[SPP_MAX_EDGE_GROUPS] = {&ga.g0, &ga.g1, &ga.g2, &ga.g3};
	for(int g = 0; g < SPP_MAX_EDGE_GROUPS; ++ g) {
		if(g < ap->n_groups)
			*gp[g] = GroupPtrs{J0[g], J1[g], Om[g], r[g], ap->edge_weights[g], (int32_t)ap->gstart[g], shape_id(ap->d0[g], ap->d1[g], ap->rd[g])};
		else
			*gp[g] = GroupPtrs{nullptr, nullptr, nullptr, nullptr, nullptr, INT32_MAX, 0};
	}
	for(int sh = 0; sh < ap->n_shapes; ++ sh) {
		const int64_t n = ap->n_shapes > 1 ? ap->n_oblist[sh] : ap->n_ob;
		const int32_t *list = ap->n_shapes > 1 ? ap->oblist[sh].p : nullptr;
		if(!n)
			continue;
#define SPP_OFFDIAG_LAUNCH(D0, D1, RD) \
		hipLaunchKernelGGL((offdiag_groups_kernel<D0, D1, RD>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, \
			n, list, ap->ob_ptr.p, ap->ob_edge.p, ap->ob_off.p, ga, vals)
		switch(gp[ap->shape_group[sh]]->shape) {
		case SHAPE_632: SPP_OFFDIAG_LAUNCH(6, 3, 2); break;
		case SHAPE_333: SPP_OFFDIAG_LAUNCH(3, 3, 3); break;
		case SHAPE_666: SPP_OFFDIAG_LAUNCH(6, 6, 6); break;
		case SHAPE_633: SPP_OFFDIAG_LAUNCH(6, 3, 3); break;
		case SHAPE_631: SPP_OFFDIAG_LAUNCH(6, 3, 1); break;
		case SHAPE_322: SPP_OFFDIAG_LAUNCH(3, 2, 2); break;
		default: break; // unary edges: no block
		}
#undef SPP_OFFDIAG_LAUNCH
	}
	bool with_633 = false, with_ext = false;
	for(int g = 0; g < ap->n_groups; ++ g) {
		with_633 = with_633 || gp[g]->shape == SHAPE_633;
		with_ext = with_ext || gp[g]->shape >= SHAPE_631;
	}
	for(int cls = 0; cls < ap->n_cls; ++ cls) {
#define SPP_VERTEX_LAUNCH(D, W633, ...) \
		if(ap->n_seq[cls]) \
			hipLaunchKernelGGL((vertex_seq_groups_kernel<D, W633, ##__VA_ARGS__>), dim3((unsigned)((ap->n_seq[cls] + 255) / 256)), dim3(256), 0, s, \
				ap->n_seq[cls], ap->vlist_seq[cls].p, ap->vl_ptr.p, ap->vl_entry.p, ap->v_doff.p, ap->v_base.p, ga, \
				ap->unary_vertex, damping, vals, eta); \
		if(ap->n_wave[cls]) \
			hipLaunchKernelGGL((vertex_wave_groups_kernel<D, W633, ##__VA_ARGS__>), dim3((unsigned)((ap->n_wave[cls] + 3) / 4)), dim3(256), 0, s, \
				ap->n_wave[cls], ap->vlist_wave[cls].p, ap->vl_ptr.p, ap->vl_entry.p, ap->v_doff.p, ap->v_base.p, ga, \
				ap->unary_vertex, damping, vals, eta);
		switch(ap->cls_dim[cls] + (with_ext ? 20 : with_633 ? 10 : 0)) {
		case 6: SPP_VERTEX_LAUNCH(6, false) break;
		case 3: SPP_VERTEX_LAUNCH(3, false) break;
		case 2: SPP_VERTEX_LAUNCH(2, false) break;
		case 16: SPP_VERTEX_LAUNCH(6, true) break;
		case 13: SPP_VERTEX_LAUNCH(3, true) break;
		case 12: SPP_VERTEX_LAUNCH(2, true) break;
		case 26: SPP_VERTEX_LAUNCH(6, true, true) break;
		case 23: SPP_VERTEX_LAUNCH(3, true, true) break;
		default: SPP_VERTEX_LAUNCH(2, true, true) break;
		}
#undef SPP_VERTEX_LAUNCH
	}
	SPP_HIP_CHECK(hipGetLastError());
}

template <int D0, int D1, int RD>
static void assemble_t(spp_ctx *ctx, const double *J0, const double *J1, const double *Om, const double *r,
	double damping, double *vals, double *eta)
{
	AssemblePlan *ap = ctx->assemble;
	hipStream_t s = ctx->stream;
	if(ap->n_ob)
		hipLaunchKernelGGL((offdiag_kernel<D0, D1, RD>), dim3((unsigned)((ap->n_ob + 255) / 256)), dim3(256), 0, s,
			ap->n_ob, ap->ob_ptr.p, ap->ob_edge.p, ap->ob_off.p, J0, J1, Om, ap->edge_weights[0], vals);
#define SPP_VERTEX_LAUNCH(D, cls) \
	if(ap->n_seq[cls]) \
		hipLaunchKernelGGL((vertex_seq_kernel<D, D0, D1, RD>), dim3((unsigned)((ap->n_seq[cls] + 255) / 256)), dim3(256), 0, s, \
			ap->n_seq[cls], ap->vlist_seq[cls].p, ap->vl_ptr.p, ap->vl_entry.p, ap->v_doff.p, ap->v_base.p, \
			J0, J1, Om, r, ap->edge_weights[0], ap->unary_vertex, damping, vals, eta); \
	if(ap->n_wave[cls]) \
		hipLaunchKernelGGL((vertex_wave_kernel<D, D0, D1, RD>), dim3((unsigned)((ap->n_wave[cls] + 3) / 4)), dim3(256), 0, s, \
			ap->n_wave[cls], ap->vlist_wave[cls].p, ap->vl_ptr.p, ap->vl_entry.p, ap->v_doff.p, ap->v_base.p, \
			J0, J1, Om, r, ap->edge_weights[0], ap->unary_vertex, damping, vals, eta);
	SPP_VERTEX_LAUNCH(D0, 0)
	if(D0 != D1) {
		SPP_VERTEX_LAUNCH(D1, 1)
	}
#undef SPP_VERTEX_LAUNCH
	SPP_HIP_CHECK(hipGetLastError());
}

void assemble_run(spp_ctx *ctx, const double *J0, const double *J1, const double *Om, const double *r,
	double damping, double *vals, double *eta)
{
	AssemblePlan *ap = ctx->assemble;
	switch(shape_id(ap->d0[0], ap->d1[0], ap->rd[0])) {
	case SHAPE_632: assemble_t<6, 3, 2>(ctx, J0, J1, Om, r, damping, vals, eta); break;
	case SHAPE_333: assemble_t<3, 3, 3>(ctx, J0, J1, Om, r, damping, vals, eta); break;
	case SHAPE_666: assemble_t<6, 6, 6>(ctx, J0, J1, Om, r, damping, vals, eta); break;
	case SHAPE_633: assemble_t<6, 3, 3>(ctx, J0, J1, Om, r, damping, vals, eta); break;
	case SHAPE_631: assemble_t<6, 3, 1>(ctx, J0, J1, Om, r, damping, vals, eta); break;
	case SHAPE_732: assemble_t<7, 3, 2>(ctx, J0, J1, Om, r, damping, vals, eta); break;
	default: assemble_t<3, 2, 2>(ctx, J0, J1, Om, r, damping, vals, eta); break;
	}
}

} // namespace spp
