// spp_sparse_plan.h -- the plan of the sparse path and the argument block of its frontal kernels, shared by the
// factorization (spp_sparse.hip), the solves on the kept factor (spp_sparse_solve.hip) and the selected inversion on it
// (spp_sparse_sigma.hip). Device units only.
#pragma once

#include "spp_internal.h"

namespace spp {

// what a workgroup of the solves on the kept factor needs of its front (spp_sparse_solve.hip)
struct AgainFront {
	int64_t off, uoff;        // offset of F in `fronts`, first row of the update panel
	int32_t h, w, ld, pad;
	int32_t row0, rowsp;      // permuted row of the first pivot, offset of the front's rows in `rows`
	int32_t cb, ce;           // its children in child_list
};

// what a workgroup of the selected inversion needs of its front and of the front's parent (spp_sparse_sigma.hip)
struct SigmaFront {
	int64_t off, poff;        // offset of the front / of its parent in `fronts` and in `sigma_z`
	int32_t h, w, ld, pad;
	int32_t pw, ppad, pld;    // the parent's pivots, padding and leading dimension (a root: 0, never read)
	int32_t relp;             // offset of the front's entries in `rel`
};

constexpr int NCLS = 5; // size classes of a front (sparse_analyze); h_cls_ptr is indexed by level * NCLS + class

struct SparsePlan {
	DevBuf<unsigned char> index_store;         // the one allocation behind the index arrays below (UploadArena)
	int64_t nb = 0, n = 0;
	int64_t n_snodes = 0, n_levels = 0;
	int64_t front_doubles = 0, vbuf_doubles = 0;
	// host
	std::vector<int32_t> h_level_ptr;          // [n_levels+1]
	std::vector<int32_t> h_front_h, h_front_w; // per supernode (scalar sizes)
	std::vector<int64_t> h_front_off;
	std::vector<int32_t> h_level_fronts;
	std::vector<int32_t> h_front_ld, h_front_pad, h_front_cls;
	std::vector<int32_t> h_cls_ptr;            // [n_levels * NCLS + 1]: fronts of (level, class) in level_fronts
	std::vector<int32_t> h_child_ptr, h_child_list, h_asm_ptr;
	std::vector<int32_t> h_front_level, h_front_parent, h_front_team; // per supernode (diagnostics: sparse_fronts)
	// device
	DevBuf<int32_t> level_fronts;              // fronts grouped by level
	DevBuf<int64_t> front_off;                 // [ns] offset of F in `fronts`
	DevBuf<int32_t> front_h, front_w, front_ld; // [ns]
	DevBuf<int32_t> front_pad;                 // [ns] identity padding inserted after the pivot block (big fronts)
	DevBuf<int64_t> front_voff;                // [ns] offset of the solve work vector
	DevBuf<int32_t> asm_ptr;                   // [ns+1]
	DevBuf<int64_t> asm_src;                   // [n_asm] (offset in vals << 1) | transpose
	DevBuf<int32_t> asm_dst;                   // [n_asm] local scalar row | local scalar col << 16
	DevBuf<int32_t> asm_shape;                 // [n_asm] dst rows | dst cols << 8
	DevBuf<int32_t> child_ptr;                 // [ns+1]
	DevBuf<int32_t> child_list;                // children in fixed (ascending) order
	DevBuf<int32_t> rel_ptr;                   // [ns+1] into rel (per supernode as a CHILD)
	DevBuf<int32_t> rel;                       // parent-local scalar index of each update row of the child
	DevBuf<int32_t> rows_ptr;                  // [ns+1]
	DevBuf<int32_t> rows;                      // permuted global scalar index of each local row
	DevBuf<int32_t> perm_scalar;               // [n] permuted scalar -> original scalar
	DevBuf<double> fronts, vbuf, xperm;
	DevBuf<int> info;
	// dependency-driven launches (front_dag_kernel): the fronts of levels < dag_level_limit, children first
	DevBuf<int32_t> front_cls, front_parent, front_level; // [ns]
	DevBuf<int32_t> dag_list, dag_list_bwd;    // dispatch order of the factorization / of the backward substitution
	DevBuf<int> dag_done;                      // [ns] epoch flags
	int32_t dag_n = 0, dag_n_bwd = 0, dag_level_limit = 0;
	int dag_solves = 0;                        // factorizations run on the team barrier counters so far
	DevBuf<int32_t> dag_rank, front_team;      // per block of the factorization launch / per front
	DevBuf<int> team_bar;                      // [ns] barrier counters of the teams (monotonic)
	DevBuf<int64_t> front_tinv;                // [ns] offset of a big front's diagonal-block inverses
	DevBuf<double> team_tinv;
	int32_t dag_first1 = 0;                    // position in dag_list of the first front of level 1
	// the levels below the first front of more than 64 rows go as a launch of their own with 256 threads and the LDS of
	// their own classes: four workgroups per CU instead of one (the wide bottom of a large tree)
	int32_t dag_split = 0, dag_split_level = 0;
	size_t dag_lds_low = 0;
	int dag_epoch = 0;
	size_t dag_lds = 0;                        // dynamic LDS of the factorization launch (largest class present)
	bool dag_ok = true;                        // false after a timed-out wait: level-by-level launches from then on
	// solves on the kept factor (spp_sparse_solve.hip): built on the first such solve
	std::vector<int64_t> h_again_uoff;         // [ns] first row of a front's update panel (h - 1 - w rows) in again_upd
	int64_t again_urows = 0;                   // rows of all update panels together
	std::vector<int32_t> h_again_rmax, h_again_hmax; // [n_levels] over the level's fronts of classes 0 - 2: largest (w | 1) (h - 1), largest h - 1
	DevBuf<int64_t> again_uoff;
	std::vector<AgainFront> h_again_desc;      // [ns] in the order of level_fronts
	DevBuf<AgainFront> again_desc;
	DevBuf<double> again_xp, again_upd;        // permuted panel (n x 128) and update panels (again_urows x 128); a pass uses 16 * NCT doubles per row
	// selected inversion on the kept factor (spp_sparse_sigma.hip): built on the first such call
	std::vector<SigmaFront> h_sigma_desc;      // [ns] in the order of level_fronts
	std::vector<int32_t> h_sigma_level;        // [n_levels * 5]: LDS doubles of the class 0 - 2 launches, their tiles of 16 update / pivot columns, the same two of classes 3 - 4
	DevBuf<SigmaFront> sigma_desc;
	DevBuf<double> sigma_z;                    // Sigma on every front's indices: front_doubles, the layout of `fronts`
};

// local (unpadded) front index -> index in a padded image: `pad` entries are inserted after the w pivots
__device__ __forceinline__ int padded(int r, int w, int pad) { return r < w ? r : r + pad; }

// the arrays of the plan the frontal kernels read (one struct: the same argument block for every kernel)
struct FrontArgs {
	const int64_t *front_off;
	const int32_t *front_h, *front_w, *front_ld, *front_pad;
	const int32_t *asm_ptr;
	const int64_t *asm_src;
	const int32_t *asm_dst, *asm_shape, *child_ptr, *child_list, *rel_ptr, *rel, *rows_ptr, *rows;
	const int64_t *front_voff;
	double *xperm;
	const double *vals;
	double *fronts, *vbuf;
	int *info;
	long long *trace; // debugging: stamps 4 (extend-add done), 5 (factored), 6 (written back) of the block's eight
};

} // namespace spp
