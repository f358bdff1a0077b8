// spp_internal.h -- private declarations shared by the translation units of libspp_hip.so.
// MI355X (gfx950) only: no CUDA shims, no CPU fallback. See include/spp_hip.h for the ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include <sys/mman.h>
#include <utility>
#include <functional>
#include <new>
#include <exception>
#include <thread>
#include <stdexcept>
#include <algorithm>
#include <string.h>
#include <chrono>
#include <stdio.h>
#include <stdlib.h>
#include "../../include/spp_hip.h"
#include "spp_switches.h"

namespace spp {

// ------------------------------------------------------------------------------------------------
// errors: internal code throws, the extern "C" layer converts to SPP_E_* codes
// ------------------------------------------------------------------------------------------------
struct Error : std::runtime_error {
	int code;
	Error(int c, const std::string &what) : std::runtime_error(what), code(c) {}
};

#define SPP_HIP_CHECK(expr) do { hipError_t e_ = (expr); if(e_ != hipSuccess) \
	throw spp::Error(SPP_E_HIP, std::string(#expr " failed: ") + hipGetErrorString(e_)); } while(0)
#define SPP_REQUIRE(cond, code, msg) do { if(!(cond)) throw spp::Error((code), (msg)); } while(0)

// hipFuncSetAttribute is per DEVICE: true the first time the calling site runs on the current device (a process may hold
// contexts on several GPUs)
inline bool first_on_this_device(uint64_t &seen)
{
	int dev = 0;
	(void)hipGetDevice(&dev);
	const uint64_t bit = uint64_t(1) << (dev & 63);
	if(seen & bit)
		return false;
	seen |= bit;
	return true;
}

// wall clock of the host-side phases of an analysis, printed lap by lap when SPP_VERBOSE is set
struct VClock {
	const char *who;
	std::chrono::steady_clock::time_point t;
	bool on;
	explicit VClock(const char *w) : who(w), t(std::chrono::steady_clock::now()), on(switches().verbose) {}
	void lap(const char *what)
	{
		if(!on)
			return;
		const std::chrono::steady_clock::time_point n = std::chrono::steady_clock::now();
		fprintf(stderr, "[spp] %s: %-34s %8.2f ms\n", who, what, std::chrono::duration<double>(n - t).count() * 1e3);
		t = n;
	}
};

// ------------------------------------------------------------------------------------------------
// device buffer (owned, grows geometrically like the reference's workspaces,
// LinearSolver_UberBlock.h:332-348)
// ------------------------------------------------------------------------------------------------
// Host arrays of the symbolic phases: tens of MB each, written once front to back. Two costs of a plain std::vector
// dominate them -- the value-initialization of resize() (a serial memset) and the first touch in 4 KB pages (63 000
// page faults per 260 MB) -- so big blocks come 2 MB-aligned and offered to transparent huge pages, and elements of
// trivial type are default-initialized (NOT zeroed: every user writes before it reads).
template <class T>
struct HugeAlloc {
	typedef T value_type;
	HugeAlloc() {}
	template <class U> HugeAlloc(const HugeAlloc<U>&) {}
	T *allocate(size_t n)
	{
		const size_t bytes = n * sizeof(T), huge = (size_t)2 << 20;
		void *q = nullptr;
		if(bytes >= ((size_t)4 << 20)) {
			if(posix_memalign(&q, huge, (bytes + huge - 1) & ~(huge - 1)) != 0)
				q = nullptr;
#ifdef MADV_HUGEPAGE
			if(q)
				madvise(q, bytes, MADV_HUGEPAGE);
#endif
		}
		if(!q)
			q = malloc(bytes ? bytes : 1);
		if(!q)
			throw std::bad_alloc();
		return (T*)q;
	}
	void deallocate(T *p, size_t) { free(p); }
	template <class U> void construct(U *p) { ::new((void*)p) U; } // default-init
	template <class U, class A0, class... A> void construct(U *p, A0 &&a0, A &&... a) { ::new((void*)p) U(std::forward<A0>(a0), std::forward<A>(a)...); }
	template <class U> bool operator==(const HugeAlloc<U>&) const { return true; }
	template <class U> bool operator!=(const HugeAlloc<U>&) const { return false; }
};
template <class T> using HVec = std::vector<T, HugeAlloc<T> >;

template <class T>
struct DevBuf {
	T *p = nullptr;
	size_t cap = 0; // elements
	bool owned = true; // false: a view into an UploadArena's single allocation
	DevBuf() {}
	DevBuf(const DevBuf&) = delete;
	DevBuf &operator=(const DevBuf&) = delete;
	~DevBuf() { release(); }
	void release()
	{
		if(p && owned)
			(void)hipFree(p);
		p = nullptr;
		cap = 0;
		owned = true;
	}
	void view(T *ptr, size_t n)
	{
		release();
		p = ptr;
		cap = n;
		owned = false;
	}
	void reserve(size_t n)
	{
		if(n <= cap && owned)
			return;
		release();
		size_t want = n;
		hipError_t e = hipMalloc((void**)&p, want * sizeof(T));
		if(e != hipSuccess) {
			p = nullptr;
			throw Error(SPP_E_NOMEM, "hipMalloc of " + std::to_string(want * sizeof(T)) + " bytes failed");
		}
		cap = want;
	}
	template <class A>
	void upload(const std::vector<T, A> &h, hipStream_t s)
	{
		reserve(h.size() ? h.size() : 1);
		if(!h.empty())
			SPP_HIP_CHECK(hipMemcpyAsync(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, s));
	}
};

// The index arrays of a plan -- a few dozen of them, kilobytes to megabytes each -- in ONE device allocation filled by ONE
// copy: a hipMalloc + a pageable-memory hipMemcpyAsync per array was most of the analysis time of a pose graph
// (26 arrays: 10-18 ms of a 14 ms sparse_analyze). add() stages a vector, commit() uploads everything and turns the
// DevBufs into views of the allocation `store` owns; the host image must live until the stream has been synchronized.
struct UploadArena {
	hipStream_t stream;
	std::vector<unsigned char> host;
	struct Item { void **pp; size_t *pcap; bool *powned; size_t off, n; };
	std::vector<Item> items;
	explicit UploadArena(hipStream_t s) : stream(s) { host.reserve(size_t(1) << 20); }
	template <class T, class A>
	void add(DevBuf<T> &b, const std::vector<T, A> &v)
	{
		if(v.size() * sizeof(T) > (size_t(256) << 10)) { // a large array gains nothing from being staged twice: its own upload
			b.upload(v, stream);
			return;
		}
		b.release();
		const size_t off = (host.size() + 255) & ~(size_t)255, bytes = std::max<size_t>(v.size(), 1) * sizeof(T);
		host.resize(off + bytes);
		if(!v.empty())
			memcpy(host.data() + off, v.data(), v.size() * sizeof(T));
		Item it = {(void**)&b.p, &b.cap, &b.owned, off, std::max<size_t>(v.size(), 1)};
		items.push_back(it);
	}
	void commit(DevBuf<unsigned char> &store)
	{
		store.release();
		store.reserve(std::max<size_t>(host.size(), 256));
		if(!host.empty())
			SPP_HIP_CHECK(hipMemcpyAsync(store.p, host.data(), host.size(), hipMemcpyHostToDevice, stream));
		for(size_t i = 0; i < items.size(); ++ i) {
			*items[i].pp = store.p + items[i].off;
			*items[i].pcap = items[i].n;
			*items[i].powned = false;
		}
	}
};

// ------------------------------------------------------------------------------------------------
// host-side copy of the analyzed Lambda structure
// ------------------------------------------------------------------------------------------------
struct Structure {
	int64_t nb = 0, n = 0, nnzb = 0, nvals = 0;
	HVec<int64_t> col_ptr, row_idx, blk_off, base;
	HVec<int32_t> dim;
};

// ------------------------------------------------------------------------------------------------
// Schur plan (guided ordering: poses first, landmarks last; LinearSolver_Schur.cpp:771-838)
// ------------------------------------------------------------------------------------------------
// one work item of the S accumulation: a chunk of the pair list of one block of S, with everything the wave
// needs to finish it in ONE 32-byte (scalar) load -- the chain of dependent fetches per item (item -> block id
// -> A offset / block coordinates -> A block) used to cost six memory round trips
struct SaccItem {
	int32_t beg, end;  // pair range
	int32_t kind;      // 0: dp x dp block of the dense S at element offset dst (leading dimension ld),
	                   // 1: contiguous dp*dp values at S + dst (sparse reduced system), 2: partial slot at partial + dst
	int32_t a_tr;      // 1: the A block is stored transposed (its cameras' positions are reversed by the camera order)
	int64_t dst;
	int64_t aoff;      // offset of the A block in vals that this item adds, or -1
};

// the scalars of a plan: what the host plan (spp_schur_plan.cpp: SchurPlanHost) and the device plan both hold
struct SchurDims {
	int dp = 0, dl = 0;            // pose / landmark block width
	int64_t nc = 0, nl = 0;        // poses, landmarks owned by this shard
	int64_t nl_total = 0;
	int64_t no = 0;                // pose-landmark blocks (observations) of this shard
	int64_t n_red = 0, ld = 0;     // reduced dimension, padded leading dimension
	int64_t n_sblk = 0;            // blocks of S that are written (upper, incl. diagonal)
	int64_t n_pairs = 0;           // sum_p k_p (k_p + 1) / 2
	int64_t n_items = 0, n_multi = 0; // work items (block chunks) / blocks split over several items
	int32_t xcd_max_items = 0;     // longest of the XCDs' item ranges (xcd_beg)
	bool u_landmark_major = true;  // layout of the packed U blocks (Up): observation order instead of camera-major
	bool factored = true;          // S accumulation on ONE packed block per observation, V = U F with C^-1 = F F^T (spp_schur.hip)
};

struct SchurPlan : SchurDims {
	bool add_A = true;             // this shard adds A and the pose rhs (rank 0)
	// reduced camera system kept SPARSE (block-CSC, dp x dp blocks) and solved by the supernodal path:
	// S buffer = [ s_st.nvals block values | n_red reduced rhs ]
	bool sparse_S = false;
	bool mis = false;              // partition by a maximal independent set instead of by block width
	Structure s_st;
	DevBuf<int64_t> sblk_voff;     // [n_sblk] offset of the S block in the sparse value array
	// host copies needed later
	std::vector<int64_t> pose_block; // reduced pose index -> original block column
	std::vector<int64_t> lm_block;   // owned landmark index -> original block column
	std::vector<uint8_t> is_lm;      // per block column: eliminated by the Schur complement (any shard)
	std::vector<uint64_t> tile_mask; // dense S: its filled 128 x 128 tile pattern over ALL shards (tile_mask_close); empty: every tile
	std::vector<int32_t> step_order; // dense S in a dissected camera order: the step order of the streamed factor (tail_step_order of tile_mask); empty: ascending
	// device arrays
	DevBuf<int32_t> lm_ptr;        // [nl+1] first obs of landmark
	DevBuf<int32_t> bs_ptr;        // [n_bs+1] landmark ranges of the fused back-substitution (at most 256 observations each); n_bs = 0: two launches
	int64_t n_bs = 0;
	int lm_stream_last = 0;        // which landmark-side kernels the last schur_form launched: 0 one lane per block, 1 / 2 the streamed forms (diagnostics: SPP_INFO_LM_STREAM)
	DevBuf<int64_t> lm_coff;       // [nl] offset of C block in vals
	DevBuf<int64_t> lm_rbase;      // [nl] scalar offset of the landmark in rhs
	DevBuf<int32_t> obs_pose;      // [no] reduced pose index
	DevBuf<int32_t> obs_lm;        // [no] owned landmark index
	DevBuf<int64_t> obs_off;       // [no] (offset in vals << 1) | transposed
	DevBuf<int64_t> pose_rbase;    // [nc] scalar offset of the pose in rhs
	DevBuf<int32_t> cam_ptr;       // [nc+1] obs list per pose (ascending landmark)
	DevBuf<int32_t> cam_obs;       // [no]
	DevBuf<int32_t> obs_wpos;      // [no] position of the observation in the per-pose (camera-major) lists:
	                               //      W, Up and xw are stored camera-major (locality of the S accumulation)
	// S accumulation work items
	DevBuf<SaccItem> items;        // [n_items] (ordered by camera tiles, not by block)
	DevBuf<int32_t> xcd_beg;       // [9] item range of each XCD (equal work, not equal counts)
	DevBuf<int32_t> sblk_i1, sblk_i2; // [n_sblk]
	DevBuf<int64_t> sblk_aoff;     // [n_sblk] offset of the A block in vals or -1; -2 - offset: the block is stored transposed
	DevBuf<int32_t> pair_a, pair_b; // [n_pairs]
	DevBuf<int32_t> multi_blk;     // [n_multi] S block id of split blocks
	DevBuf<int32_t> multi_ptr;     // [n_multi+1] slot range
	// numeric workspaces
	DevBuf<double> cinv;           // [nl * dl*dl]   -(C^-1)
	DevBuf<double> lfac;           // [nl * dl*dl]   F = chol(C)^-T, upper triangular, C^-1 = F F^T (factored form)
	DevBuf<double> W;              // [no * dp*dl]   -U C^-1, camera-major
	DevBuf<double> Up;             // [no * dp*dl]   U packed, camera-major
	DevBuf<double> xw;             // [no * dp]      W l per observation
	DevBuf<double> partial;        // [slots * dp*dp]
	DevBuf<double> S;              // [ld*ld + ld] when the caller does not supply the buffer
	// A tile of S outside the filled mask is zero whenever a factorization starts: true while that is NOT known of the
	// buffer S (after its allocation, and after any factorization on it other than the fully masked streamed launch,
	// which never writes a tile without a workgroup). schur_form then clears the whole buffer, else the listed tiles.
	bool unlisted_dirty = true;
	// the side stream of schur_form (SPP_SCHUR_SIDE) has work the ctx stream has not waited for yet; padding and status
	// reset of the coming factorization are already enqueued there
	bool side_pending = false, side_padded = false;
	int side_last = 0, clear_last = 0; // diagnostics of the last schur_form: SPP_INFO_SCHUR_SIDE, SPP_INFO_S_CLEAR
	// the last spp_factor_solve_device left a factor a further solve may use (dense S in the own buffer, unsharded, SPP_OK):
	// R in S, the whole block inverses in dense.tinv_all. Cleared on entry of every call that rewrites any of it (SPP_INFO_FACTOR_KEPT)
	bool factor_kept = false;
	// spp_schur_sigma_device (spp_schur_sigma.hip), made on its first call for this plan: Z = S^-1 (ld x ld, both triangles) and
	// the stored camera-camera blocks of Lambda as (offset in vals, row camera's position, column camera's position)
	DevBuf<double> sigma_Z;
	DevBuf<int64_t> sigma_cc;
	std::vector<int64_t> sigma_cc_host;
	int64_t sigma_ncc = -1;        // -1: the list has not been made
	// the last spp_factor_solve_device left the factor of the SPARSE reduced system in the fronts of the sparse plan (sparse_S, no
	// independent-set cut, unsharded, SPP_OK); set and cleared where factor_kept is (SPP_INFO_SCHUR_SPARSE_FACTOR_KEPT)
	bool sparse_factor_kept = false;
	// spp_schur_sparse_sigma_device (spp_schur_sparse_sigma.hip), made on its first call for this plan: the blocks of Z = S^-1
	// on the stored pattern of S (s_st.nvals doubles in the layout sblk_voff indexes) and S's block-CSC lists
	DevBuf<double> sigma_Zb;
	DevBuf<int64_t> sigma_scol, sigma_srow; // s_st.col_ptr [nc + 1], s_st.row_idx [n_sblk]
	int async_last = 0;           // ... of the last schur_finish: 1 = it returned on the factor's status with the stream still running (SPP_SOLVE_ASYNC), 0 = it drained the stream (SPP_INFO_SOLVE_ASYNC)
	void release_all();
};

// ------------------------------------------------------------------------------------------------
// the streamed launch of the dense factor (spp_dense_tail.h): what the host decides for it (tail_plan, spp_tile_plan.cpp)
// ------------------------------------------------------------------------------------------------
constexpr int TAIL_MAX_ROWS = 64; // tile columns of a region: one bit each in a step's word
constexpr int TAIL_NO_STEP = 127; // (no tile row: a tile applies the steps below its own row only)
constexpr int TAIL_SORDER_WORDS = TAIL_MAX_ROWS / 8 + 1;

// The step list of a launch, one byte per step, eight to a word (entry p in byte p & 7 of sorder[p >> 3]): the step as a
// signed byte -- -1: the row panel in front of the region --, TAIL_NO_STEP behind the last one.
__host__ __device__ inline int tail_sorder_at(const unsigned long long *sorder, const int p)
{
	return (int)(signed char)(unsigned char)(sorder[p >> 3] >> (8 * (p & 7)));
}

inline void tail_sorder_pack(unsigned long long *sorder, const int *list, const int n) // (entries behind list[n - 1]: TAIL_NO_STEP)
{
	for(int p = 0; p < 8 * TAIL_SORDER_WORDS; ++ p) {
		if(!(p & 7))
			sorder[p >> 3] = 0;
		sorder[p >> 3] |= (unsigned long long)(unsigned char)(signed char)(p < n ? list[p] : TAIL_NO_STEP) << (8 * (p & 7));
	}
}

struct TailSwitches { // the run-time switches a plan depends on, as values (the host probes vary them within one process)
	int tail_rows, tail_mask, tail_early, tail_early_lead;
	double tail_order_beta;
	static TailSwitches of(const Switches &sw) { return TailSwitches{sw.tail_rows, sw.tail_mask, sw.tail_early, sw.tail_early_lead, sw.tail_order_beta}; }
};

struct TailPlan {
	bool applies = false;  // false: the region is not one streamed launch (the per-step schedule goes on); nothing below is set
	// what the workgroup table is a function of (beside the order key's beta and the resident count, fixed for a device)
	struct Key {
		int Tr = 0, Tc = 0;            // tile rows / tile columns of the region
		bool have_pre = false;         // a row panel in front of the region (step -1)
		bool early = false;            // the caller's mask in force and SPP_TAIL_EARLY: lagging trailing rows may go first
		bool lead = false;             // ... the leading rows of a run that is too large (tail_order_table's lead)
		// the step words: bit j of rowbits[i + 1] = tile (i, j) of the region is nonzero, rowbits[0] = the row panel in front
		std::vector<uint64_t> rowbits;
		bool operator ==(const Key &o) const
		{
			return Tr == o.Tr && Tc == o.Tc && have_pre == o.have_pre && early == o.early && lead == o.lead && rowbits == o.rowbits;
		}
	} key;
	bool masked = false;   // the caller's tile mask is in force (else every tile is listed)
	bool ordered = false;  // the step list is the caller's step order (else ascending)
	unsigned long long sorder[TAIL_SORDER_WORDS]; // the step list (-1 first with have_pre), packed
	int resident = 0;      // resident workgroups the table was made for (0 unless early)
	bool table_fresh = false; // the table was computed by this call (false: taken over from a former plan with the same key)
	std::vector<int> table; // workgroup -> tile (i << 16 | j)
	int info[5] = {0, 0, 0, 0, 0}; // tail_order_table's figures of that table
};

// ------------------------------------------------------------------------------------------------
// dense Cholesky workspace
// ------------------------------------------------------------------------------------------------
struct DenseWork {
	DevBuf<double> tinv;           // inverse of the current diagonal block (NB x NB)
	DevBuf<int> info;              // device flag: 0 ok, j+1 = pivot j non-positive
	DevBuf<double> tinv_all;       // inverses of all diagonal blocks (nblk x NB x NB) kept for the solves
	int64_t tinv_half = 0;         // > 0: that many of them are in the two-halves form the factorization leaves (completed before a solve)
	DevBuf<double> xtmp;           // solution of the backward substitution before it replaces y
	DevBuf<int> flags;             // per block row: epoch of the solve that last published x_b (chain kernel)
	DevBuf<int> tail_pub;          // streamed tail of the dense factor: per tile, (epoch << 4) | row tiles published
	DevBuf<double> tail_dinv;      // ... and the inverse 16 x 16 diagonal tiles it publishes
	int tail_epoch = 0;
	DevBuf<int> tail_order;        // workgroup -> tile of the streamed launch: tail_plan.table on the device
	TailPlan tail_plan;            // the plan of the last streamed launch; its table is the host image of tail_order (the upload is asynchronous: it lives as long as the table)
	int tail_resident = -1;       // workgroups of the streamed launch the device holds at once (occupancy x CUs); -1: not asked yet
	// Tile structure of the matrix the next factorization gets (set by the caller for that one call, TileMaskGuard): one
	// word per tile row of 128, bit j = tile (i, j) is nonzero after symbolic fill (tile_mask_close). nullptr or a size
	// that does not match the factorization's tile rows: every tile is nonzero.
	const std::vector<uint64_t> *tile_mask = nullptr;
	// The order in which the tiles of the next factorization apply their steps, when the whole of it is ONE streamed launch
	// (set with the mask, TileMaskGuard): a permutation of its tile rows. nullptr or another size: ascending. It changes
	// the summation order, so -- unlike the mask -- it holds whatever SPP_TAIL_MASK says.
	const std::vector<int32_t> *step_order = nullptr;
	bool tail_masked_whole = false; // the last factorization was ONE streamed launch (no per-step front) under the caller's tile mask
	int tail_rows_last = 0;        // tile rows the last factorization streamed (diagnostics: SPP_INFO_DENSE_STREAMED)
	bool tail_disabled = false;    // a streamed launch timed out on this ctx: later factorizations take the per-step schedule
	DevBuf<double> trsv_m;         // M_b = Tinv_b R_{b, b+1} per block row (M form of the backward substitution)
	DevBuf<double> trsv_pay;       // hand-over pairs {value, check word} of the one-workgroup chain: x (nblk x 128) and w (nblk x 128)
	DevBuf<double> trsm_w;         // multi-column solves (spp_dense_trsm.h): the panel of finished blocks, nblk * 128 rows x 128 columns
	uint64_t epoch = 0;            // solves so far (backward-substitution chains tell one solve from the next by it)
	int *h_chain_err = nullptr;    // timeout word of the chain kernels: page-locked, mapped host memory they store into on their error path alone (dense_chain_check)
	int *d_chain_err = nullptr;    // ... its device address
	bool chain_disabled = false;   // a chain kernel timed out on this ctx: later backward substitutions launch per block row
	hipStream_t aux = nullptr;     // lookahead stream: potrf_diag + trsm of the next panel
	hipEvent_t ev[2] = {nullptr, nullptr};
	// device-flag hand-offs between the chain stream and the bulk stream (dense_factor_steps_enqueue):
	// sync[2 k] = row panel k complete, sync[2 k + 1] = bulk update k complete, as the epoch of the factorization
	DevBuf<int> sync;
	DevBuf<int> fuse_cnt;          // per step: sub-tiles of the next diagonal tile finished (update_potrf_kernel)
	std::vector<int> fuse_expect;  // host: the value every counter will have reached behind the launches enqueued so far
	bool fuse_dirty = false;       // counters and bookkeeping disagree (aborted factorization): cleared before the next use
	int64_t ident_from = -1;       // >= 0: the pivots from this index on are exact identity padding (set around a call by the sparse path)
	// lookahead factorization (spp_dense_la.h): persistent chain kernel on its own stream (CU-masked to the reserved CUs),
	// counters of one factorization, and whether the chain / bulk stream pair was seen to run concurrently
	hipStream_t chain = nullptr;
	hipEvent_t ev_chain = nullptr;
	DevBuf<int> la_cnt;
	DevBuf<long long> la_trace;
	int la_state = 0;              // 0: untested, 1: usable, -1: off
	int la_reserve = 0;            // CUs kept free of the bulk stream (= workgroups the chain kernel may have)
	int la_ncu = 0;
	int sync_epoch = 0;
	int sync_state = 0;            // 0: not tested on this stream, 1: the streams run concurrently, -1: disabled
	hipStream_t sync_stream = nullptr; // the ctx stream the self-test ran against
};

// ------------------------------------------------------------------------------------------------
// sparse (multifrontal supernodal) plan -- spp_sparse.hip / spp_symbolic.cpp
// ------------------------------------------------------------------------------------------------
struct SparsePlan;

// ------------------------------------------------------------------------------------------------
// assembly plan -- spp_assemble.hip
// ------------------------------------------------------------------------------------------------
struct AssemblePlan;

struct PhaseTimer {
	hipEvent_t ev[2 * SPP_N_PHASES];
	bool used[SPP_N_PHASES];
	bool created = false;
};

} // namespace spp

struct spp_ctx {
	int device = 0;
	int flags = 0;
	hipStream_t stream = nullptr;
	bool own_stream = false;
	// Schur stage: what the S accumulation does not feed (reduced rhs, padding, status reset) runs here beside it; forked
	// from / joined into `stream` by the two events (created on first use, spp_schur.hip). Not dense.aux: that one is
	// CU-masked and belongs to the per-step schedule of the dense factor.
	hipStream_t side_stream = nullptr;
	hipEvent_t side_ev[2] = {nullptr, nullptr};
	// Solve stage (SPP_SOLVE_ASYNC): the factor's four status words travel to h_status (page-locked) on the side stream,
	// forked from `stream` behind the factor by status_ev[0]; the host waits for status_ev[1], recorded behind the copy, and
	// for nothing else. Both are re-recorded only after that wait.
	hipEvent_t status_ev[2] = {nullptr, nullptr};
	int *h_status = nullptr;
	bool status_pending = false; // a copy was enqueued and the host has not waited for it (a call that failed in between)
	std::string last_error;
	int mode = -1; // -1: not analyzed
	int shard_rank = 0, shard_world = 1;
	spp::Structure st;
	std::vector<int64_t> order; // elimination order (block columns)
	std::thread plan_trash; // releases the host image of the last Schur plan (hundreds of MB) beside the caller; joined by the next analysis and by spp_destroy
	spp::SchurPlan schur;
	spp::DenseWork dense;
	spp::SparsePlan *sparse = nullptr;
	spp::AssemblePlan *assemble = nullptr;
	// staging buffers for the host-pointer entry points
	spp::DevBuf<double> d_vals, d_rhs;
	double *h_staging = nullptr; // page-locked host buffer handed out by spp_host_staging()
	size_t h_staging_cap = 0;    // doubles
	// spp_solve_device (spp_solve_again.hip): the camera panel of a pass (ld x 128); kept_marginals (either kept factor): the
	// unit block columns and the selected rows of a covariance (the host image lives as long as its asynchronous upload may run)
	spp::DevBuf<double> again_panel, again_cols;
	spp::DevBuf<int64_t> again_rows;
	std::vector<int64_t> again_rows_host;
	// spp_sparse_solve_device / spp_sparse_marginals_device / spp_sparse_sigma_device: the fronts of the sparse plan hold the
	// factor of the last spp_factor_solve_device (SPP_MODE_SPARSE, SPP_OK) and nothing has rewritten them since
	bool sparse_factor_kept = false;
	spp::DevBuf<double> geom_partial; // partial sums of ||dx||^2 (spp_geometry.hip)
	// profiling
	spp::PhaseTimer timer;
	double phase_ms[SPP_N_PHASES] = {0};
	// dominant-kernel accounting (MFMA trailing update)
	std::vector<hipEvent_t> dom_events; // pairs
	size_t dom_used = 0;
	double dom_flops = 0;
	int64_t factor_flops = 0, solve_bytes = 0, factor_nnz = 0;
};

namespace spp {

// ---- spp_geometry.hip ----
void se2_linearize(spp_ctx *ctx, int64_t ne, const int32_t *d_v0, const int32_t *d_v1, const double *d_poses,
	const double *d_meas, double *d_J0, double *d_J1, double *d_r);
double se2_update(spp_ctx *ctx, int64_t nv, double *d_poses, const double *d_dx, bool apply);
void se2_linearize_at(spp_ctx *ctx, int64_t ne, const int64_t *d_off0, const int64_t *d_off1, const double *d_state,
	const double *d_meas, double *d_J0, double *d_J1, double *d_r);
void se2_rb_linearize(spp_ctx *ctx, int64_t ne, const int64_t *d_off0, const int64_t *d_off1, const double *d_state,
	const double *d_meas, double *d_J0, double *d_J1, double *d_r);
double slam2d_update(spp_ctx *ctx, int64_t n, double *d_state, const double *d_dx, int64_t n_angles,
	const int64_t *d_angle_off, bool apply);
void se3_linearize_at(spp_ctx *ctx, int64_t ne, const int64_t *d_off0, const int64_t *d_off1, const double *d_state,
	const double *d_meas, double *d_J0, double *d_J1, double *d_r);
void se3_xyz_linearize(spp_ctx *ctx, int64_t ne, const int64_t *d_pose_off, const int64_t *d_lm_off, const double *d_state,
	const double *d_meas, double *d_J0, double *d_J1, double *d_r);
double slam3d_update(spp_ctx *ctx, int64_t n, double *d_state, const double *d_dx, int64_t n_poses,
	const int64_t *d_pose_off, bool apply);
void rocv_range_linearize(spp_ctx *ctx, int64_t ne, const int64_t *d_recv_off, const int64_t *d_lm_off, const double *d_state,
	const double *d_meas, double *d_J0, double *d_J1, double *d_r);
void rocv_cv_linearize(spp_ctx *ctx, int64_t ne, const int64_t *d_off0, const int64_t *d_off1, const double *d_state,
	const double *d_dt, double *d_J0, double *d_J1, double *d_r);
double edge_chi2(spp_ctx *ctx, int64_t ne, int rd, const double *d_r, const double *d_Om);
void edge_robust_weights(spp_ctx *ctx, int64_t ne, int rd, int kind, double scale, double param, const double *d_r, double *d_w);
double edge_hessian_maxdiag(spp_ctx *ctx, int64_t ne, int rd, int d0, int d1, const double *d_J0, const double *d_J1,
	const double *d_Om);
double lm_gain_denominator(spp_ctx *ctx, int64_t n, const double *d_dx, const double *d_rhs, double alpha);
void se3_linearize(spp_ctx *ctx, int64_t ne, const int32_t *d_v0, const int32_t *d_v1, const double *d_poses,
	const double *d_meas, double *d_J0, double *d_J1, double *d_r);
double se3_update(spp_ctx *ctx, int64_t nv, double *d_poses, const double *d_dx, bool apply);
void ba_linearize(spp_ctx *ctx, int64_t no, const int32_t *d_cam_of, const int32_t *d_pt_of, const double *d_cams,
	const double *d_intr, const double *d_pts, const double *d_meas, double *d_J0, double *d_J1, double *d_r);
void ba_stereo_linearize(spp_ctx *ctx, int64_t no, const int32_t *d_cam_of, const int32_t *d_pt_of, const double *d_cams,
	const double *d_intr, const double *d_pts, const double *d_meas, double *d_J0, double *d_J1, double *d_r);
void ba_intrinsics_linearize(spp_ctx *ctx, int64_t no, const int32_t *d_cam_of, const int32_t *d_pt_of, const int32_t *d_intr_of,
	const double *d_cams, const double *d_intr, const double *d_pts, const double *d_meas, double *d_J0, double *d_J1, double *d_J2,
	double *d_r);
double ba_intrinsics_update(spp_ctx *ctx, int64_t ni, double *d_intr, const int64_t *d_intr_dxoff, const double *d_dx, bool apply);
double ba_update(spp_ctx *ctx, int64_t nc, double *d_cams, const int64_t *d_cam_dxoff, int64_t np, double *d_pts,
	const int64_t *d_pt_dxoff, const double *d_dx, int64_t n_dx, bool apply);
void sim3_ba_linearize(spp_ctx *ctx, int64_t no, const int32_t *d_cam_of, const int32_t *d_pt_of, const double *d_cams,
	const double *d_intr, const double *d_pts, const double *d_meas, double *d_J0, double *d_J1, double *d_r);
double sim3_update(spp_ctx *ctx, int64_t nc, double *d_cams, const int64_t *d_cam_dxoff, int64_t np, double *d_pts,
	const int64_t *d_pt_dxoff, const double *d_dx, int64_t n_dx, bool apply);

// ---- spp_symbolic.cpp ----
void min_degree_order(int64_t nb, const int64_t *col_ptr, const int64_t *row_idx, std::vector<int64_t> &order);
void nested_dissection_order(int64_t nb, const int64_t *col_ptr, const int64_t *row_idx, std::vector<int64_t> &order);

// ---- spp_tile_plan.cpp (host-side tile planning of the dense factor) ----
// Tile masks of an n x n matrix (+ right-hand side column n) in 128 x 128 tiles (host only).
// tile_mask_mark: the tiles the bs x bs blocks (i1[q], i2[q]) at rows / columns bs * index touch (either triangle given,
// the upper one marked); words is resized to the tile rows, or left EMPTY (= every tile) with more than 64 tile columns.
// tile_mask_close: diagonal tiles and the right-hand side's tile column set, nothing below the diagonal, then symbolic
// elimination (for k ascending every pair of nonzero tiles (k, a), (k, b), k < a <= b, fills (a, b)); returns the
// number of rank-128 tile updates of the filled pattern.
void tile_mask_mark(int64_t n, int bs, int64_t nblk, const int32_t *i1, const int32_t *i2, std::vector<uint64_t> &words);
int64_t tile_mask_close(int64_t n, bool has_rhs, bool fill, std::vector<uint64_t> &words);
// Cost model of the streamed launch on a filled tile mask (host only: tile_dag_cost). The launch is
// bound by its chain of diagonal tiles or by its tile updates, whichever is longer:
//   cost = max(path * TAIL_MODEL_STEP_US, updates * TAIL_MODEL_UPDATE_US / resident) + TAIL_MODEL_START_US.
// The constants are the measured ones of DESIGN sections 10 - 11 (profiles/r04_dense_tail_trace.txt, r06_dense_tail_trace.txt):
// a step of the chain = 31 - 34 us of potrf_diag panels + 3 - 5 us of hand-over = 36.5 us; a tile applies a row tile
// in 2.0 us when it only streams (2.6 us while it catches up, 4.6 us is the rate at which the chain emits them); the
// launch starts 45 us before its first step ends; 256 resident workgroups (one per CU of an MI355X) -- a constant and
// not the device's count, so that every rank and every host probe chooses the same camera order.
constexpr double TAIL_MODEL_STEP_US = 36.5, TAIL_MODEL_UPDATE_US = 2.0, TAIL_MODEL_START_US = 45.0;
constexpr int TAIL_MODEL_RESIDENT = 256;
struct TileDagCost {
	int64_t tiles = 0, updates = 0, path = 0; // listed tiles, rank-128 updates, longest chain of diagonal tiles
	double cost_us = 0;
};
TileDagCost tile_dag_cost(int64_t n, const std::vector<uint64_t> &filled, int resident); // (filled: tile_mask_close(n, true, true))
// workgroup -> tile (i << 16 | j) of the streamed launch for the step words bits[0 .. Tr] of a region (host only; the rule
// and the progress condition are stated at its definition)
// lead: where the trailing run is too large to be seated whole, its leading rows are (used together with a step order)
void tail_order_table(const std::vector<uint64_t> &bits, int Tr, int Tc, bool have_pre, double beta, int resident, bool early,
	std::vector<int> &order, int *info, bool lead = false);
// Everything the host decides for a streamed launch (host only, no device call; stated at its definition): the region behind
// step k (-1: the whole factorization) of a factorization of nsteps tile rows, `rows` pivot rows and ncols columns; mask
// (may be null): the caller's filled mask, one word per tile row; step_order (may be null): the caller's step order;
// resident: workgroups the device holds at once. former (may be null): a plan whose table is taken over -- moved, its
// storage stays where it is -- when the key is the same; no table is computed then. Throws SPP_E_BADARG for a step order
// that is no permutation.
TailPlan tail_plan(const std::vector<uint64_t> *mask, const std::vector<int32_t> *step_order, int64_t nsteps, int64_t rows,
	int64_t ncols, int64_t k, int resident, const TailSwitches &sw, TailPlan *former = nullptr);
bool is_permutation(const int32_t *v, int64_t n); // v[0 .. n) holds every value 0 .. n - 1 once
// the order in which a tile of the streamed launch applies its steps: by the depth of the step's diagonal tile in the
// tile DAG of the filled mask (one word per tile row), ties by k (host only; stated at its definition)
void tail_step_order(const std::vector<uint64_t> &filled, std::vector<int32_t> &order);

// ---- spp_schur_plan.cpp ----
void build_schur_plan(spp_ctx *ctx, bool sparse_S, bool mis = false);
int64_t schur_buffer_doubles(const spp_ctx *ctx); // S | rhs buffer the Schur entry points work on
bool schur_applicable(const Structure &st, int *dp, int *dl);
double schur_plan_host_probe(const Structure &st, int shard_rank, int shard_world, bool sparse_S, bool mis, int64_t *out); // host only: plan + its two checksums (out[0..8]), seconds
void schur_tile_mask_host_probe(const Structure &st, std::vector<uint64_t> &words); // the mask a dense Schur plan carries in the NATURAL camera order
// host only: the camera order the Schur plan of a structure and shard uses, read back from that plan (cam_order[position] = camera in natural numbering)
// and the model's figures of the natural order / of that order; order_in given: the figures of THAT order in cost[1],
// nothing is chosen. Returns whether cam_order differs from the identity.
bool schur_cam_order_host_probe(const Structure &st, int shard_rank, int shard_world, bool sparse_S, bool mis, const int64_t *order_in,
	std::vector<int32_t> &cam_order, TileDagCost cost[2]);
// host only: the step order the Schur plan of a structure and shard hands to the streamed factor, read back from that plan
// (one entry per tile row of S, the identity where the plan carries none; empty without a tile mask). Returns whether
// the plan carries one.
bool schur_step_order_host_probe(const Structure &st, int shard_rank, int shard_world, bool sparse_S, bool mis, std::vector<int32_t> &step_order);

// ---- spp_sparse (symbolic on host + numeric on device) ----
void sparse_analyze(spp_ctx *ctx, const Structure &st); // plan for `st` (Lambda, or the sparse reduced system)
int sparse_factor_solve(spp_ctx *ctx, const double *d_vals, double *d_rhs);
void sparse_release(spp_ctx *ctx);
void sparse_dag_disable(spp_ctx *ctx); // after a timed-out flag wait: level-by-level launches from then on
int64_t sparse_info(const spp_ctx *ctx, int what);
int64_t sparse_fronts(const spp_ctx *ctx, int64_t capacity, int32_t *h, int32_t *w, int32_t *pad, int32_t *cls, int32_t *level,
	int32_t *parent, int32_t *team);

// ---- spp_schur.hip ----
// Observations from which on schur_form forks the side stream (SPP_SCHUR_SIDE=1). The fork and the join are one barrier
// packet each on the ctx stream, ~6 us apiece on this runtime, 12 us together; rhs_kernel takes 6.1 us
// at 31 843 observations (Ladybug-49, profiles/r03_ladybug49_kernel_stats.csv: the launch floor) and 63.8 us at 2 838 740
// (Venice-871, profiles/r08_venice871_kernel_stats.csv). Between the two it reaches the 12 us of the hand-overs near
// 300 000 observations; the threshold keeps a margin above that.
constexpr int64_t SCHUR_SIDE_MIN_OBS = 500000;
// one_call: spp_factor_solve_device runs (schur_finish follows on the same stream and takes over the join with the side stream)
void schur_form(spp_ctx *ctx, const double *d_vals, const double *d_rhs, double *d_S_rhs, bool one_call = false);
int schur_finish(spp_ctx *ctx, const double *d_vals, double *d_S_rhs, double *d_rhs);
void schur_pack(spp_ctx *ctx, double *S, double *packed, bool pack);

// ---- spp_solve_again.hip ----
// Lambda X = B in place for nrhs columns (n rows in Lambda's numbering, leading dimension ldb) against the kept factor
void schur_solve_again(spp_ctx *ctx, const double *d_vals, double *d_B, int64_t ldb, int64_t nrhs);
// the same against the kept factor of the sparse reduced system: the camera panel goes through sparse_solve_again
void schur_sparse_solve_again(spp_ctx *ctx, const double *d_vals, double *d_B, int64_t ldb, int64_t nrhs);
// E^T Lambda^-1 E of the selected vertices (block columns of Lambda), m x m, exactly symmetric, on whichever kept factor
// `solve` works: solve(d_B, ldb, nrhs) is Lambda X = B in place on the ctx's stream. `who` names the entry point in the
// error texts.
typedef std::function<void(double *d_B, int64_t ldb, int64_t nrhs)> KeptSolve;
void kept_marginals(spp_ctx *ctx, const char *who, int64_t n_sel, const int64_t *h_vertices, double *d_cov, const KeptSolve &solve);

// ---- spp_schur_sigma.hip ----
// the blocks of Lambda^-1 on the stored pattern of Lambda (the layout of vals) from the kept dense Schur factor;
// dense_only: form Z = S^-1 in the plan's workspace and stop (what tools/schur_sigma_time.py times as the dense part)
void schur_sigma(spp_ctx *ctx, const double *d_vals, double *d_sigma, bool dense_only = false);

// ---- spp_sparse_solve.hip ----
// Lambda X = B in place for nrhs columns (n rows in Lambda's numbering, leading dimension ldb) against the fronts the last
// sparse factorization left in the plan
void sparse_solve_again(spp_ctx *ctx, double *d_B, int64_t ldb, int64_t nrhs);

// ---- spp_sparse_sigma.hip ----
// the blocks of Lambda^-1 on the stored pattern of Lambda (the layout of vals) from the fronts the last sparse
// factorization left in the plan
void sparse_sigma(spp_ctx *ctx, double *d_sigma);
// its two halves: the recursion down the assembly tree into the plan's second arena, and the gather of the stored blocks
// of the factored matrix out of that arena into `dst` (the layout of that matrix's value array)
void sparse_sigma_arena(spp_ctx *ctx);
void sparse_sigma_gather(spp_ctx *ctx, double *dst);

// ---- spp_schur_sparse_sigma.hip ----
// the blocks of Lambda^-1 on the stored pattern of Lambda (the layout of vals) from the kept factor of the sparse reduced
// system; inverse_only: the blocks of Z = S^-1 into the plan's workspace and stop (tools/schur_sparse_again_time.py)
void schur_sparse_sigma(spp_ctx *ctx, const double *d_vals, double *d_sigma, bool inverse_only = false);

// ---- spp_dense.hip ----
constexpr int DENSE_NB = 128;
int dense_potrf_upper(spp_ctx *ctx, double *d_A, int64_t n, int64_t ld, bool keep_inverses);
// returns whether the whole factorization went to the streamed launch under the caller's tile mask (the one schedule that
// leaves every tile outside the mask untouched); info_reset false: the caller has enqueued dense_info_reset_on() itself
bool dense_potrf_upper_enqueue(spp_ctx *ctx, double *d_A, int64_t n, int64_t ld, bool info_reset = true);
int dense_info_fetch(spp_ctx *ctx, bool *dag_aborted = nullptr); // dag_aborted given: a timed-out sparse launch is reported there instead of thrown
// its two halves, for a caller that lets other work run between them: the copy of the four status words to h_status4
// (page-locked) on a stream the caller orders behind the factorization, and -- once the host has waited for that copy --
// what dense_info_fetch makes of them. drain_first: words that are not all zero (a failed pivot, a timed-out wait) are
// acted on only after the ctx stream was synchronized, as in dense_info_fetch
void dense_info_copy_on(spp_ctx *ctx, hipStream_t st, int *h_status4);
int dense_info_eval(spp_ctx *ctx, const int *h_status4, bool *dag_aborted = nullptr, bool drain_first = false);
void dense_potrs_upper(spp_ctx *ctx, const double *d_R, int64_t n, int64_t ld, double *d_b);
// R^T R X = B in place for nrhs columns against the factor and the block inverses of the last factorization (spp_dense_trsm.h)
void dense_potrs_multi(spp_ctx *ctx, const double *d_R, int64_t n, int64_t ld, double *d_B, int64_t ldb, int64_t nrhs);
void dense_tinv_complete(spp_ctx *ctx); // the stored block inverses in their whole form (no-op when they are)
// Z (n x n, leading dimension ldz, both triangles, exactly symmetric) <- (R^T R)^-1 against the same (spp_dense_potri.h)
void dense_potri_upper(spp_ctx *ctx, const double *d_R, int64_t n, int64_t ld, double *d_Z, int64_t ldz);
void dense_aux_park(int device, hipStream_t s); // hands the bulk stream of a closing context to the next one
void dense_factor_steps(spp_ctx *ctx, double *d_A, int64_t ld, int64_t n, int64_t rows, int64_t ncols,
	int64_t nsteps, bool has_rhs);
void dense_info_reset(spp_ctx *ctx);
void dense_info_ensure(spp_ctx *ctx); // the status words exist (created and zeroed on the ctx stream)
void dense_info_reset_on(spp_ctx *ctx, hipStream_t st); // ... reset on a stream the caller orders against the ctx stream
void dense_reserve(spp_ctx *ctx, int64_t nblk); // workspaces for nblk diagonal blocks (call at analyze time)

// call after the stream was synchronized. The chain kernels store their timeout word straight into page-locked host
// memory (DenseWork::h_chain_err), so a timed-out chain is reported by the first call that synchronizes with its solve:
// spp_synchronize, spp_memcpy_d2h, a draining entry point, or the next solve's status wait
void dense_chain_check(spp_ctx *ctx);
void dense_set_padding(spp_ctx *ctx, double *d_A, int64_t ld, int64_t n);
void dense_set_padding_on(hipStream_t st, double *d_A, int64_t ld, int64_t n);
struct TileMaskGuard { // hands a tile mask (and a step order) to the factorizations enqueued while it lives
	DenseWork &d;
	TileMaskGuard(DenseWork &dw, const std::vector<uint64_t> *m, const std::vector<int32_t> *so = nullptr) : d(dw)
	{
		d.tile_mask = (m && !m->empty()) ? m : nullptr;
		d.step_order = (so && !so->empty()) ? so : nullptr;
	}
	~TileMaskGuard() { d.tile_mask = nullptr; d.step_order = nullptr; }
};
// unit tests: the partial factorization of a big sparse front, laid out (identity padding after the w pivots) and
// factored as the sparse path does; d_F (h x h, ld) <- the result in the unpadded layout, d_image (optional, ldp x hp with
// ldp = (hp + 1) & ~1, hp = h + pad) <- the padded image
int dense_front_factor(spp_ctx *ctx, double *d_F, int64_t ld, int64_t w, int64_t h, double *d_image);
bool dense_gemm_tn_sub(spp_ctx *ctx, int64_t m, int64_t n, int64_t k, const double *A, int64_t lda,
	const double *B, int64_t ldb, double *C, int64_t ldc, bool upper_only);
double microbench_copy(spp_ctx *ctx, size_t bytes, int iters);
double microbench_mfma_f64(spp_ctx *ctx, int iters);
double microbench_ctile(spp_ctx *ctx, int n, int iters);
double microbench_update(spp_ctx *ctx, int64_t m, int iters);

// ---- spp_assemble.hip ----
// one plan type: spp_assemble_analyze is the one-group case (g_seq null: the groups concatenated in group order)
void assemble_analyze(spp_ctx *ctx, int64_t nv, const int32_t *dim, int n_groups, const int64_t *g_ne,
	const int64_t *const *g_v0, const int64_t *const *g_v1, const int64_t *const *g_seq, const int *g_d0, const int *g_d1,
	const int *g_rd, int64_t unary_vertex, const uint8_t *skip_vertex = nullptr); // skip_vertex[v]: v enters no vertex list
int assemble_n_groups(const spp_ctx *ctx);
int64_t assemble_group_edges(const spp_ctx *ctx, int group);
bool assemble_group_is_unary(const spp_ctx *ctx, int group); // unary edges: no second vertex, J1 unused
void assemble_run(spp_ctx *ctx, const double *J0, const double *J1, const double *Om, const double *r,
	double damping, double *vals, double *eta); // plans of one group
void assemble_groups_run(spp_ctx *ctx, const double *const *J0, const double *const *J1, const double *const *Om,
	const double *const *r, double damping, double *vals, double *eta); // host arrays of n_groups device pointers
void assemble_set_edge_weights(spp_ctx *ctx, int group, const double *d_w); // null: plain edges
void assemble_release(spp_ctx *ctx);
bool assemble_is_ternary(const spp_ctx *ctx);
// ---- spp_assemble3.hip ----
constexpr int ASM_HUB_CHUNK = 4096; // edges one workgroup of the hub reduction sums (SPP_INFO_ASM_HUB_CHUNK)
void assemble_analyze_ternary(spp_ctx *ctx, int64_t nv, const int32_t *dim, int64_t ne, const int64_t *v0, const int64_t *v1,
	const int64_t *v2, int64_t unary_vertex);
void assemble_ternary_run(spp_ctx *ctx, const double *J0, const double *J1, const double *J2, const double *Om, const double *r,
	double damping, double *vals, double *eta);
void assemble_get_structure(const spp_ctx *ctx, int64_t *col_ptr, int64_t *row_idx, int64_t *blk_off);

// ---- profiling helpers (spp_api.cpp) ----
void phase_begin(spp_ctx *ctx, int phase);
void phase_end(spp_ctx *ctx, int phase);
void phases_reset(spp_ctx *ctx);
void phases_collect(spp_ctx *ctx);
// dominant-kernel event bracket
void dom_begin(spp_ctx *ctx);
void dom_end(spp_ctx *ctx, double flops);

// ---- host threads of the symbolic phases (spp_schur_plan.cpp, spp_assemble.hip)
// Runs fn(t) for t = 0 .. nt-1 on nt host threads (fn(0) on the caller's). The symbolic phase is integer work over
// tens of millions of block products; its passes are cut into independent pieces with precomputed output offsets, so
// the result does not depend on the number of threads.
template <class F>
inline void run_threads(int nt, F fn)
{
	if(nt <= 1) {
		fn(0);
		return;
	}
	std::vector<std::thread> th;
	std::exception_ptr err[64];
	for(int t = 1; t < nt; ++ t)
		th.emplace_back([&, t]() { try { fn(t); } catch(...) { err[t] = std::current_exception(); } });
	try { fn(0); } catch(...) { err[0] = std::current_exception(); }
	for(size_t t = 0; t < th.size(); ++ t)
		th[t].join();
	for(int t = 0; t < nt; ++ t)
		if(err[t])
			std::rethrow_exception(err[t]);
}

inline int plan_threads(int64_t work)
{
	const int env = switches().plan_threads; // 0: automatic
	int nt = env ? env : (int)std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency()));
	if(work < switches().plan_min_work)
		nt = 1; // small problems: a thread costs more than it saves
	return std::min(nt, 64);
}

// cut [0, n) into nt pieces of about equal weight; w_prefix has n + 1 entries (w_prefix[0] = 0)
template <class V>
inline void balanced_cuts(const V &w_prefix, int nt, std::vector<int64_t> &cut)
{
	const int64_t n = (int64_t)w_prefix.size() - 1, total = w_prefix[n];
	cut.assign(nt + 1, n);
	cut[0] = 0;
	for(int t = 1; t < nt; ++ t)
		cut[t] = std::lower_bound(w_prefix.begin(), w_prefix.end(), total * t / nt) - w_prefix.begin();
	for(int t = 1; t <= nt; ++ t)
		cut[t] = std::max(cut[t], cut[t - 1]);
	cut[nt] = n;
}


} // namespace spp
