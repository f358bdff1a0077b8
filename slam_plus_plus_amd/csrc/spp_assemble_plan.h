// spp_assemble_plan.h -- the assembly plan and the per-edge device bodies shared by spp_assemble.hip (binary edges) and
// spp_assemble3.hip (ternary edges: the binary kernels write what does not touch an intrinsics vertex, the border
// kernels the rest).
#pragma once

#include "spp_internal.h"

namespace spp {

// One plan type for one edge group and for several: edges are numbered through the concatenation of the groups
// (group g holds the indices gstart[g] .. gstart[g + 1)), every list below holds such indices in ascending GLOBAL position
// (h_seq of spp_assemble_analyze_groups; the concatenation itself without it). With one group and no h_seq that is the
// edge index itself: the lists are then those the one-group kernels have always read.
constexpr int MAX_WIDTH_CLASSES = 3; // distinct vertex widths of one plan's shapes (6, 3, 2; a (7,3,2) plan holds 7 and 3 alone)

// The border of a plan of ternary edges (camera, point, intrinsics; spp_assemble3.hip): every destination that touches an
// intrinsics vertex. Destinations are numbered kind by kind -- H02 blocks (camera, intrinsics), H12 blocks (point,
// intrinsics), then one per intrinsics vertex (H22 and g2) --, each with the list of its edges in ascending order.
struct TernaryPlan {
	enum { K02 = 0, K12 = 1, K22 = 2, N_KINDS = 3 };
	int64_t n_dst = 0, n_chunks = 0, n_hub = 0;
	DevBuf<unsigned char> index_store;
	DevBuf<int32_t> dst_ptr;    // [n_dst+1] range of the destination in dst_edge
	DevBuf<int32_t> dst_edge;   // [3 ne] edge indices, ascending inside a destination
	DevBuf<int64_t> dst_off;    // [n_dst] offset in vals of the block (K22: the diagonal block)
	DevBuf<int64_t> dst_eoff;   // [n_dst] K22: scalar offset in eta; else unused
	DevBuf<int32_t> dst_flags;  // [n_dst] bit 0: the block is stored transposed (intrinsics id below the other); K22: the unary factor
	DevBuf<int32_t> seq_list[N_KINDS];   // destinations of at most SEQ_MAX_DEGREE edges
	int64_t n_seq[N_KINDS] = {0};
	DevBuf<int32_t> chunk_dst[N_KINDS];  // hub reduction, stage 1: destination of every chunk ...
	DevBuf<int32_t> chunk_beg[N_KINDS];  // ... its first position in dst_edge (ASM_HUB_CHUNK positions, or to the end of the list) ...
	DevBuf<int32_t> chunk_slot[N_KINDS]; // ... and its slot in `partial`
	int64_t n_chunk[N_KINDS] = {0};
	DevBuf<int32_t> hub_dst, hub_kind, hub_slot_ptr; // stage 2: [n_hub] destination and kind, [n_hub+1] slot range (ascending chunk order)
	DevBuf<double> partial;     // [n_chunks * HUB_STRIDE]
};

struct AssemblePlan {
	TernaryPlan *ternary = nullptr; // the plan is one of ternary edges: the lists below are those of its (camera, point) part
	~AssemblePlan() { delete ternary; }
	int n_groups = 1;
	int d0[SPP_MAX_EDGE_GROUPS] = {0}, d1[SPP_MAX_EDGE_GROUPS] = {0}, rd[SPP_MAX_EDGE_GROUPS] = {0}; // d1 = 0: a group of unary edges
	int64_t gstart[SPP_MAX_EDGE_GROUPS + 1] = {0};
	int n_cls = 0, cls_dim[MAX_WIDTH_CLASSES] = {0}; // vertex width classes, in order of first appearance (d0, d1 of group 0, ...)
	int n_shapes = 0, shape_group[SPP_MAX_EDGE_GROUPS] = {0}; // distinct (d0, d1, rd): the first group of each
	int64_t nv = 0, ne = 0, unary_vertex = -1;
	Structure st;
	int64_t n_ob = 0;
	DevBuf<unsigned char> index_store; // the one allocation behind the index arrays below (UploadArena)
	DevBuf<int32_t> ob_ptr;     // [n_ob+1]
	DevBuf<int32_t> ob_edge;    // edge | reversed << 31
	DevBuf<int64_t> ob_off;     // [n_ob] offset of the block in vals
	DevBuf<int32_t> vl_ptr;     // [nv+1]
	DevBuf<int32_t> vl_entry;   // edge << 1 | side
	DevBuf<int64_t> v_doff;     // [nv] offset of the diagonal block
	DevBuf<int64_t> v_base;     // [nv] scalar offset in eta
	DevBuf<int32_t> vlist_seq[MAX_WIDTH_CLASSES], vlist_wave[MAX_WIDTH_CLASSES];
	int64_t n_seq[MAX_WIDTH_CLASSES] = {0}, n_wave[MAX_WIDTH_CLASSES] = {0};
	DevBuf<int32_t> oblist[SPP_MAX_EDGE_GROUPS]; // off-diagonal blocks of each shape (more than one shape only; else all of them)
	int64_t n_oblist[SPP_MAX_EDGE_GROUPS] = {0};
	// device, one robust weight per edge of the group, or null (assemble_set_edge_weights; not owned)
	const double *edge_weights[SPP_MAX_EDGE_GROUPS] = {nullptr};
};

constexpr int SEQ_MAX_DEGREE = 24; // a destination fed by at most that many edges is summed by one thread, in edge order

#ifdef __HIPCC__
// T = J^T Omega  (D x RD), J is RD x D column-major
template <int D, int RD>
__device__ __forceinline__ void jt_omega(const double *__restrict__ J, const double *__restrict__ Om, double *T)
{
#pragma unroll
	for(int c = 0; c < RD; ++ c)
#pragma unroll
		for(int i = 0; i < D; ++ i) {
			double s = 0;
#pragma unroll
			for(int l = 0; l < RD; ++ l)
				s += J[l + i * RD] * Om[l + c * RD];
			T[i + c * D] = s;
		}
}

// contribution of one (edge, side) to the vertex: H (D x D, upper computed, mirrored) and g (D)
template <int D, int RD, int SIDE>
__device__ __forceinline__ void vertex_contrib(const double *__restrict__ J, const double *__restrict__ Om,
	const double *__restrict__ r, double wgt, double *H, double *g)
{
	// wgt: the robust weight of the edge (1 for a plain edge: the products below are then exact), applied where the
	// reference applies it (BaseTypes_Binary.h:768-848): side 0 through T = J0^T Omega w -- H00 carries it once, g0 = T r w
	// TWICE --, side 1 on the finished H11 and g1
	double T[D * RD];
	jt_omega<D, RD>(J, Om, T);
	if(SIDE == 0) {
#pragma unroll
		for(int i = 0; i < D * RD; ++ i)
			T[i] *= wgt;
	}
#pragma unroll
	for(int c = 0; c < D; ++ c)
#pragma unroll
		for(int i = 0; i <= c; ++ i) {
			double s = 0;
#pragma unroll
			for(int l = 0; l < RD; ++ l)
				s += T[i + l * D] * J[l + c * RD];
			H[i + c * D] = (SIDE == 0) ? s : s * wgt;
		}
	if(SIDE == 0) { // g0 = (J0^T Omega) r
#pragma unroll
		for(int i = 0; i < D; ++ i) {
			double s = 0;
#pragma unroll
			for(int l = 0; l < RD; ++ l)
				s += T[i + l * D] * r[l];
			g[i] = s * wgt;
		}
	} else {        // g1 = J1^T (Omega r)
		double orr[RD];
#pragma unroll
		for(int l = 0; l < RD; ++ l) {
			double s = 0;
#pragma unroll
			for(int m = 0; m < RD; ++ m)
				s += Om[l + m * RD] * r[m];
			orr[l] = s;
		}
#pragma unroll
		for(int i = 0; i < D; ++ i) {
			double s = 0;
#pragma unroll
			for(int l = 0; l < RD; ++ l)
				s += J[l + i * RD] * orr[l];
			g[i] = s * wgt;
		}
	}
}

#endif // __HIPCC__

} // namespace spp
