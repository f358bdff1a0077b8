// spp_schur_plan.cpp -- the symbolic Schur plan (host side, integer work, once per block structure).
//
//  schur_applicable / build_schur_plan: the guided Schur ordering and everything the reference recomputes structurally
//  in every CLinearSolver_Schur::Solve_PosDef_Blocky call
//      n_Calculate_GuidedOrdering      include/slam/LinearSolver_Schur.h:2154-2207, src/slam/LinearSolver_Schur.cpp:771-838
//      Permute_UpperTriangular_To      src/slam/BlockMatrix.cpp:8183 (replaced by index indirection: no data moves)
//      SliceTo x3 + TransposeTo        include/slam/LinearSolver_Schur.h:1699-1709 (replaced by the obs / pair lists)
//      symbolic part of MultiplyToWith src/slam/BlockMatrixFBS.inl:1147-1304 (the S block pattern + pair lists)
//  The plan itself, schur_plan_host(), is a sequence of phases over one SchurPlanHost (the result) and one PlanScratch
//  (what crosses phases without being part of the result); build_schur_plan() uploads it, the three *_host_probe
//  functions reach it without a device.

#include "spp_internal.h"
#include <sys/mman.h>
#include <stdlib.h>
#include <algorithm>
#include <numeric>
#include <string.h>
#include <stdio.h>
#include <thread>
#include <memory>
#include <chrono>
#include <exception>

namespace spp {

void SchurPlan::release_all()
{
	lm_ptr.release(); bs_ptr.release(); n_bs = 0; lm_coff.release(); lm_rbase.release(); obs_pose.release(); obs_lm.release();
	obs_off.release(); pose_rbase.release(); cam_ptr.release(); cam_obs.release(); items.release();
	obs_wpos.release(); xcd_beg.release(); sblk_i1.release(); sblk_i2.release(); sblk_aoff.release();
	sblk_voff.release(); s_st = Structure(); sparse_S = false; mis = false;
	pair_a.release(); pair_b.release(); multi_blk.release(); multi_ptr.release(); cinv.release(); lfac.release();
	W.release(); Up.release(); xw.release(); partial.release(); S.release();
	pose_block.clear(); lm_block.clear(); is_lm.clear(); tile_mask.clear(); step_order.clear();
	sigma_Z.release(); sigma_cc.release(); sigma_cc_host.clear(); sigma_ncc = -1;
	sigma_Zb.release(); sigma_scol.release(); sigma_srow.release();
}

// Guided ordering is possible when there are exactly two block widths and the blocks of the
// smaller width (landmarks) are not connected to each other (C block diagonal). Mirrors
// LinearSolver_Schur.h:1586-1594 (fall back when there are not two vertex dimensions) and
// :1721-1726 (the fast path requires b_BlockDiagonal()).
bool schur_applicable(const Structure &st, int *dp_out, int *dl_out)
{
	int d_a = -1, d_b = -1;
	for(int64_t j = 0; j < st.nb; ++ j) {
		int d = st.dim[j];
		if(d_a < 0 || d == d_a) d_a = d;
		else if(d_b < 0 || d == d_b) d_b = d;
		else return false;
	}
	if(d_a < 0 || d_b < 0)
		return false;
	int dp = std::max(d_a, d_b), dl = std::min(d_a, d_b);
	if(!((dp == 6 && dl == 3) || (dp == 3 && dl == 2) || (dp == 7 && dl == 3)))
		return false; // kernel instantiations (BA: SE3 pose + XYZ; 2D SLAM: SE2 pose + XY; Sim(3) BA: Sim3 camera + XYZ)
	int64_t n_lm = 0;
	for(int64_t j = 0; j < st.nb; ++ j) {
		if(st.dim[j] == dl)
			++ n_lm;
		for(int64_t p = st.col_ptr[j]; p < st.col_ptr[j + 1]; ++ p) {
			int64_t i = st.row_idx[p];
			if(i != j && st.dim[i] == dl && st.dim[j] == dl)
				return false; // landmark-landmark block: C not block diagonal
		}
	}
	if(n_lm == 0)
		return false;
	*dp_out = dp;
	*dl_out = dl;
	return true;
}

static const int PAIR_CHUNK = 2048; // pairs per work item of the S accumulation

int64_t schur_buffer_doubles(const spp_ctx *ctx)
{
	const SchurPlan &sp = ctx->schur;
	return sp.sparse_S ? sp.s_st.nvals + sp.n_red : sp.ld * sp.ld;
}

// Maximum-independent-set cut for graphs of ONE block width (the general ordering of the reference,
// CSchurOrdering, src/slam/LinearSolver_Schur.cpp:690-769,1235-1340): vertices of the independent set play the
// landmarks' role (their diagonal part C is block diagonal by construction), the rest forms the reduced
// system. Greedy by ascending degree (ties by index): deterministic, maximal, not maximum.
static bool mis_partition(const Structure &st, std::vector<uint8_t> &is_lm, int *d_out)
{
	const int d = st.dim[0];
	for(int64_t j = 0; j < st.nb; ++ j)
		if(st.dim[j] != d)
			return false;
	if(d != 3 && d != 6)
		return false;
	std::vector<std::vector<int32_t> > adj(st.nb);
	for(int64_t j = 0; j < st.nb; ++ j)
		for(int64_t p = st.col_ptr[j]; p < st.col_ptr[j + 1]; ++ p) {
			const int64_t i = st.row_idx[p];
			if(i != j) {
				adj[i].push_back((int32_t)j);
				adj[j].push_back((int32_t)i);
			}
		}
	std::vector<int32_t> order(st.nb);
	for(int64_t j = 0; j < st.nb; ++ j)
		order[j] = (int32_t)j;
	std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return adj[a].size() < adj[b].size(); });
	is_lm.assign(st.nb, 0);
	std::vector<uint8_t> blocked(st.nb, 0);
	int64_t n_lm = 0;
	for(int64_t q = 0; q < st.nb; ++ q) {
		const int32_t v = order[q];
		if(blocked[v])
			continue;
		is_lm[v] = 1;
		++ n_lm;
		for(size_t e = 0; e < adj[v].size(); ++ e)
			blocked[adj[v][e]] = 1;
	}
	*d_out = d;
	return n_lm > 0 && n_lm < st.nb;
}

// uninitialized host array (a std::vector would zero-fill -- and page-fault -- 100 MB on one thread)
template <class T>
struct RawBuf {
	T *p = nullptr;
	size_t n = 0;
	RawBuf() {}
	RawBuf(const RawBuf&) = delete;
	RawBuf &operator=(const RawBuf&) = delete;
	~RawBuf() { free(p); }
	void resize(size_t m)
	{
		free(p);
		p = nullptr;
		if(m) {
			// big work arrays (tens of MB, written once front to back): 2 MB-aligned and offered to transparent huge pages --
			// first touch of 260 MB in 4 KB pages is 63 000 page faults, a third of the pair-list phase
			const size_t bytes = m * sizeof(T);
			if(bytes >= ((size_t)8 << 20)) {
				void *q = nullptr;
				if(posix_memalign(&q, (size_t)2 << 20, (bytes + (((size_t)2 << 20) - 1)) & ~(((size_t)2 << 20) - 1)) == 0) {
					p = (T*)q;
#ifdef MADV_HUGEPAGE
					madvise(q, bytes, MADV_HUGEPAGE);
#endif
				}
			}
			if(!p)
				p = (T*)malloc(bytes);
			if(!p)
				throw std::bad_alloc();
		}
		n = m;
	}
	size_t size() const { return n; }
	T &operator[](size_t i) { return p[i]; }
	const T &operator[](size_t i) const { return p[i]; }
};

// the tiles of S = A - sum over landmarks of U C^-1 U^T, over the landmarks of ALL shards (the exchanged S is the sum
// over the ranks): every camera-camera block of the structure and, per eliminated block, every pair of its observers
static void schur_tile_mask(const Structure &st, const std::vector<uint8_t> &is_lm, const std::vector<int32_t> &pose_of,
	int dp, int64_t n_red, std::vector<uint64_t> &words)
{
	tile_mask_mark(n_red, dp, 0, nullptr, nullptr, words);
	if(words.empty())
		return;
	const int64_t Tr = (int64_t)words.size();
	auto tiles_of = [&](int32_t pose) -> uint64_t {
		return (1ull << ((int64_t)pose * dp / DENSE_NB)) | (1ull << (((int64_t)pose * dp + dp - 1) / DENSE_NB));
	};
	auto mark = [&](uint64_t rows, const uint64_t cols) {
		for(; rows; rows &= rows - 1) {
			const int a = __builtin_ctzll(rows);
			if(a < Tr)
				words[a] |= cols;
		}
	};
	std::vector<uint64_t> seen(st.nb, 0); // per eliminated block: the tiles of its observers
	for(int64_t j = 0; j < st.nb; ++ j)
		for(int64_t p = st.col_ptr[j]; p < st.col_ptr[j + 1]; ++ p) {
			const int64_t i = st.row_idx[p];
			if(!is_lm[i] && !is_lm[j])
				mark(tiles_of(pose_of[i]), tiles_of(pose_of[j])), mark(tiles_of(pose_of[j]), tiles_of(pose_of[i])); // (either sense: a camera order may reverse the two; tile_mask_close keeps the upper one)
			else if(!is_lm[i])
				seen[j] |= tiles_of(pose_of[i]);
			else if(!is_lm[j])
				seen[i] |= tiles_of(pose_of[j]);
		}
	for(int64_t j = 0; j < st.nb; ++ j)
		if(seen[j])
			mark(seen[j], seen[j]);
	tile_mask_close(n_red, true, true, words);
}

// --------------------------------------------------------------------------------------------------
// Camera order of a dense reduced system. The streamed dense factor is bound by its chain of
// diagonal tiles; in the natural order of a closed camera loop (a band plus a wrap-around border) every tile row k has
// tile (k - 1, k), so the chain is all tile rows. Ordered arc A, arc B, separators -- A and B not co-visible, B starting
// on a tile boundary -- no listed tile couples the arcs and the shorter arc's diagonal tiles are factored beside the
// longer one's.
// --------------------------------------------------------------------------------------------------
// co-visibility of the cameras in their natural numbering, a row of bits per camera (camera-camera blocks, pairs of
// observers of an eliminated block, the camera itself); over the landmarks of ALL shards, like the tile mask
struct CamGraph {
	int64_t nc = 0, nw = 0;
	std::vector<uint64_t> bits;
	uint64_t *row(int64_t c) { return bits.data() + c * nw; }
	const uint64_t *row(int64_t c) const { return bits.data() + c * nw; }
};

static void cam_graph(const Structure &st, const std::vector<uint8_t> &is_lm, const std::vector<int32_t> &cam_of, int64_t nc, CamGraph &g)
{
	g.nc = nc;
	g.nw = (nc + 63) / 64;
	g.bits.assign((size_t)(nc * g.nw), 0);
	auto set = [&](int64_t a, int64_t b) { g.row(a)[b >> 6] |= 1ull << (b & 63); };
	// observers per eliminated block (counting sort: an observation lies in the column of whichever of the two comes later)
	std::vector<int64_t> ptr((size_t)st.nb + 1, 0);
	for(int64_t j = 0; j < st.nb; ++ j)
		for(int64_t p = st.col_ptr[j]; p < st.col_ptr[j + 1]; ++ p) {
			const int64_t i = st.row_idx[p];
			if(is_lm[i] != is_lm[j])
				++ ptr[(is_lm[i] ? i : j) + 1];
		}
	for(int64_t j = 0; j < st.nb; ++ j)
		ptr[j + 1] += ptr[j];
	std::vector<int32_t> obs((size_t)ptr[st.nb]);
	{
		std::vector<int64_t> fill(ptr.begin(), ptr.end() - 1);
		for(int64_t j = 0; j < st.nb; ++ j)
			for(int64_t p = st.col_ptr[j]; p < st.col_ptr[j + 1]; ++ p) {
				const int64_t i = st.row_idx[p];
				if(!is_lm[i] && !is_lm[j]) {
					set(cam_of[i], cam_of[j]);
					set(cam_of[j], cam_of[i]);
				} else if(is_lm[i] != is_lm[j])
					obs[fill[is_lm[i] ? i : j] ++] = cam_of[is_lm[i] ? j : i];
			}
	}
	// every observer's row takes the block's observer set (only the words it spans). Ranges of blocks on host threads, each
	// into an image of its own (nc^2 bits: 93 KB at 871 cameras), the images are OR-ed afterwards
	const int nt = plan_threads((int64_t)obs.size() * 4);
	std::vector<int64_t> lcut;
	balanced_cuts(ptr, nt, lcut);
	std::vector<std::vector<uint64_t> > img((size_t)nt);
	run_threads(nt, [&](int t) {
		std::vector<uint64_t> &im = img[t];
		im.assign(g.bits.size(), 0);
		std::vector<uint64_t> tmp((size_t)g.nw, 0);
		for(int64_t l = lcut[t]; l < lcut[t + 1]; ++ l) {
			const int64_t b = ptr[l], e = ptr[l + 1];
			if(b == e)
				continue;
			int64_t lo = g.nw, hi = -1;
			for(int64_t q = b; q < e; ++ q) {
				const int64_t w = obs[q] >> 6;
				tmp[w] |= 1ull << (obs[q] & 63);
				lo = std::min(lo, w);
				hi = std::max(hi, w);
			}
			for(int64_t q = b; q < e; ++ q) {
				uint64_t *r = im.data() + obs[q] * g.nw;
				for(int64_t w = lo; w <= hi; ++ w)
					r[w] |= tmp[w];
			}
			for(int64_t w = lo; w <= hi; ++ w)
				tmp[w] = 0;
		}
	});
	for(int t = 0; t < nt; ++ t)
		for(size_t q = 0; q < g.bits.size(); ++ q)
			g.bits[q] |= img[t][q];
	for(int64_t c = 0; c < nc; ++ c)
		set(c, c);
}

// the filled tile mask of the graph with camera c at position pos[c] (what schur_tile_mask gives for that order)
static void cam_graph_mask(const CamGraph &g, const std::vector<int32_t> &pos, int dp, int64_t n_red, std::vector<uint64_t> &words)
{
	tile_mask_mark(n_red, dp, 0, nullptr, nullptr, words);
	if(words.empty())
		return;
	const int64_t Tr = (int64_t)words.size();
	std::vector<uint64_t> tl((size_t)g.nc);
	for(int64_t c = 0; c < g.nc; ++ c)
		tl[c] = (1ull << ((int64_t)pos[c] * dp / DENSE_NB)) | (1ull << (((int64_t)pos[c] * dp + dp - 1) / DENSE_NB));
	for(int64_t c = 0; c < g.nc; ++ c) {
		uint64_t cols = 0;
		const uint64_t *r = g.row(c);
		for(int64_t w = 0; w < g.nw; ++ w)
			for(uint64_t m = r[w]; m; m &= m - 1)
				cols |= tl[w * 64 + __builtin_ctzll(m)];
		for(uint64_t rows = tl[c]; rows; rows &= rows - 1) {
			const int a = __builtin_ctzll(rows);
			if(a < Tr)
				words[a] |= cols;
		}
	}
	tile_mask_close(n_red, true, true, words);
}

// whether the streamed launch keeps its progress margin on this mask: the live-demand condition of tail_order_table
static bool cam_order_live_ok(const std::vector<uint64_t> &filled, int64_t n_red)
{
	// (the whole factorization as one launch under the mask, k ascending, on the model's device)
	const TailSwitches sw = {TAIL_MAX_ROWS, 1, 1, 0, 0.0};
	const TailPlan p = tail_plan(&filled, nullptr, (int64_t)filled.size(), n_red, n_red + 1, -1, TAIL_MODEL_RESIDENT, sw);
	return p.applies && (p.info[0] > 0 || p.info[3] <= TAIL_MODEL_RESIDENT); // the trailing rows are seated early, or everything live fits
}

// The rule. A LOOP is cut only: the first and the last camera of the natural order are co-visible (the natural order is
// then a band plus a wrap-around border, and that border is a separator already). Candidates: arc A = the cameras
// [a, a + m) of the natural order, m a multiple of the cameras between two tile boundaries; separator = the cameras A
// sees -- on a loop, two runs --, B = all the others (so no block couples A and B), in one connected piece, cut down to a
// whole number of tiles (its last cameras join the separator). An open chain, an arrow or two components keep the
// natural order. The candidate that hides the most tile rows (the shorter of the two arcs is the longest) is taken, ties:
// the smaller separator, B in one run of the natural order, the smaller m, a. Inside A, B and the separator the cameras
// keep their natural order. Accepted only if the model's cost falls by a tenth and the live-demand condition holds;
// otherwise order = identity. order[position] = camera.
static bool cam_dissect(const CamGraph &g, int dp, int64_t n_red, std::vector<int32_t> &order, TileDagCost cost[2])
{
	const int64_t nc = g.nc, nw = g.nw;
	order.resize((size_t)nc);
	std::vector<int32_t> pos((size_t)nc);
	for(int64_t c = 0; c < nc; ++ c)
		order[c] = pos[c] = (int32_t)c;
	std::vector<uint64_t> words;
	cam_graph_mask(g, pos, dp, n_red, words);
	if(words.empty())
		return false;
	cost[0] = cost[1] = tile_dag_cost(n_red, words, TAIL_MODEL_RESIDENT);
	int64_t al = DENSE_NB;
	for(int64_t x = dp, y = DENSE_NB; y; ) { // al = 128 / gcd(128, dp) cameras
		const int64_t t = x % y;
		x = y;
		y = t;
		if(!y)
			al = DENSE_NB / x;
	}
	typedef std::vector<uint64_t> Set;
	auto count = [&](const Set &x) { int64_t n = 0; for(int64_t w = 0; w < nw; ++ w) n += __builtin_popcountll(x[w]); return n; };
	auto nbrs = [&](const Set &x, Set &out) { // union of the rows of x
		out.assign((size_t)nw, 0);
		for(int64_t w = 0; w < nw; ++ w)
			for(uint64_t m = x[w]; m; m &= m - 1) {
				const uint64_t *r = g.row(w * 64 + __builtin_ctzll(m));
				for(int64_t v = 0; v < nw; ++ v)
					out[v] |= r[v];
			}
	};
	auto flood = [&](const Set &within, Set &comp) { // comp (a seed inside `within`) <- its connected piece of `within`
		Set front(comp), nb;
		for(;;) {
			nbrs(front, nb);
			bool grew = false;
			for(int64_t w = 0; w < nw; ++ w) {
				front[w] = nb[w] & within[w] & ~comp[w];
				comp[w] |= front[w];
				grew = grew || front[w];
			}
			if(!grew)
				return;
		}
	};
	auto first_bit = [&](const Set &x, Set &seed) {
		seed.assign((size_t)nw, 0);
		for(int64_t w = 0; w < nw; ++ w)
			if(x[w]) {
				seed[w] = x[w] & (~x[w] + 1);
				return true;
			}
		return false;
	};
	Set all((size_t)nw, 0);
	for(int64_t c = 0; c < nc; ++ c)
		all[c >> 6] |= 1ull << (c & 63);
	if(!((g.row(0)[(nc - 1) >> 6] >> ((nc - 1) & 63)) & 1))
		return false; // the natural order does not close on itself: no loop
	struct Cand { int64_t shorter = 0, sep = 0, runs = 0, a = 0, m = 0; } best;
	Set A((size_t)nw), S, B((size_t)nw), bestA, bestB, comp;
	const int64_t stride = std::max<int64_t>(1, al / 8);
	for(int64_t m = al; 2 * m <= nc; m += al)
		for(int64_t a = 0; a + m <= nc; a += stride) {
			std::fill(A.begin(), A.end(), 0);
			for(int64_t c = a; c < a + m; ++ c)
				A[c >> 6] |= 1ull << (c & 63);
			nbrs(A, S);
			for(int64_t w = 0; w < nw; ++ w) {
				S[w] &= ~A[w];
				B[w] = all[w] & ~A[w] & ~S[w];
			}
			const int64_t nB = count(B), nBal = nB - nB % al;
			if(nBal == 0)
				continue;
			Cand cd;
			cd.shorter = std::min(m, nBal);
			cd.sep = nc - m - nBal;
			cd.a = a;
			cd.m = m;
			for(int64_t c = 0; c < nc; ++ c) // runs of consecutive cameras in B
				cd.runs += ((B[c >> 6] >> (c & 63)) & 1) && !(c && ((B[(c - 1) >> 6] >> ((c - 1) & 63)) & 1));
			if(best.m && !(cd.shorter > best.shorter || (cd.shorter == best.shorter && (cd.sep < best.sep ||
			   (cd.sep == best.sep && cd.runs < best.runs)))))
				continue; // (a and m ascend: the earlier candidate wins a full tie)
			// B in one piece (an arrow or a second component would fall apart)
			first_bit(B, comp);
			flood(B, comp);
			if(comp != B)
				continue;
			best = cd;
			bestA = A;
			bestB = B;
		}
	if(switches().verbose)
		fprintf(stderr, "[spp] camera order: best arc a %lld m %lld shorter %lld sep %lld runs %lld\n", (long long)best.a,
			(long long)best.m, (long long)best.shorter, (long long)best.sep, (long long)best.runs);
	if(!best.m)
		return false;
	// positions: A, the first whole tiles of B, everything else; natural order inside each
	const int64_t nBal = count(bestB) - count(bestB) % al;
	std::vector<int32_t> cand_order;
	cand_order.reserve((size_t)nc);
	std::vector<uint8_t> placed((size_t)nc, 0);
	for(int64_t c = 0; c < nc; ++ c)
		if((bestA[c >> 6] >> (c & 63)) & 1) {
			cand_order.push_back((int32_t)c);
			placed[c] = 1;
		}
	for(int64_t c = 0, k = 0; c < nc && k < nBal; ++ c)
		if((bestB[c >> 6] >> (c & 63)) & 1) {
			cand_order.push_back((int32_t)c);
			placed[c] = 1;
			++ k;
		}
	for(int64_t c = 0; c < nc; ++ c)
		if(!placed[c])
			cand_order.push_back((int32_t)c);
	for(int64_t q = 0; q < nc; ++ q)
		pos[cand_order[q]] = (int32_t)q;
	cam_graph_mask(g, pos, dp, n_red, words);
	const TileDagCost c1 = tile_dag_cost(n_red, words, TAIL_MODEL_RESIDENT);
	const bool live_ok = cam_order_live_ok(words, n_red);
	if(switches().verbose)
		fprintf(stderr, "[spp] camera order: candidate tiles %lld updates %lld chain %lld model %.0f us (natural %.0f), live ok %d\n",
			(long long)c1.tiles, (long long)c1.updates, (long long)c1.path, c1.cost_us, cost[0].cost_us, (int)live_ok);
	if(!(c1.cost_us <= 0.9 * cost[0].cost_us) || !live_ok)
		return false;
	cost[1] = c1;
	order.swap(cand_order);
	return true;
}

// the camera order of a plan: cam_order[position] = camera in natural numbering (cam_of[block column])
static bool schur_cam_order(const Structure &st, const std::vector<uint8_t> &is_lm, const std::vector<int32_t> &cam_of, int64_t nc,
	int dp, bool sparse_S, bool mis, const int64_t *order_in, std::vector<int32_t> &cam_order, TileDagCost cost[2])
{
	cam_order.resize((size_t)nc);
	for(int64_t c = 0; c < nc; ++ c)
		cam_order[c] = (int32_t)c;
	cost[0] = cost[1] = TileDagCost();
	const int64_t n_red = nc * dp;
	// only where the streamed factor can work on a tile mask: dense S, at most 64 tile columns. (Not tied to SPP_TAIL_MASK:
	// that switch promises the same bits with and without the mask, tests/test_gpu_dense_tilemask.py, so the order must
	// not depend on it.)
	if(sparse_S || mis || n_red / DENSE_NB + 1 > 64 || nc < 2 || (!order_in && !switches().schur_cam_order))
		return false;
	VClock clk("camera order");
	CamGraph g;
	cam_graph(st, is_lm, cam_of, nc, g);
	clk.lap("co-visibility graph");
	if(order_in) { // (probe: the model's figures of a given order)
		std::vector<int32_t> pos((size_t)nc);
		for(int64_t q = 0; q < nc; ++ q) {
			cam_order[q] = (int32_t)order_in[q];
			pos[order_in[q]] = (int32_t)q;
		}
		std::vector<uint64_t> words;
		for(int side = 0; side < 2; ++ side) {
			if(!side)
				for(int64_t c = 0; c < nc; ++ c)
					pos[c] = (int32_t)c;
			else
				for(int64_t q = 0; q < nc; ++ q)
					pos[order_in[q]] = (int32_t)q;
			cam_graph_mask(g, pos, dp, n_red, words);
			cost[side] = tile_dag_cost(n_red, words, TAIL_MODEL_RESIDENT);
		}
		return false;
	}
	const bool used = cam_dissect(g, dp, n_red, cam_order, cost);
	clk.lap("dissection + cost model");
	return used;
}

// Everything build_schur_plan() derives from the block structure, in host memory: the pure symbolic part (no device,
// no ctx), also reachable through spp_schur_plan_host() for host-only tests and timing.
struct SchurPlanHost : SchurDims {
	int64_t n_ablk = 0;
	int32_t n_slots = 0;
	std::vector<int64_t> pose_block, lm_block;
	std::vector<uint8_t> is_lm;
	HVec<int32_t> lm_ptr, obs_pose, obs_lm, cam_obs, wpos; // (per observation / landmark: HVec = not zero-filled, huge pages)
	std::vector<int32_t> bs_ptr; // landmark ranges of at most BS_OBS observations (fused back-substitution); empty: a landmark has more
	std::vector<int32_t> cam_ptr, sblk_i1, sblk_i2, multi_blk, multi_ptr, xb;
	RawBuf<int32_t> pair_a, pair_b; // (tens of millions of entries: not value-initialized, first touched by the threads that fill them)
	HVec<int64_t> lm_coff, obs_off, lm_rbase;
	std::vector<int64_t> sblk_aoff, sblk_voff, pose_rbase;
	std::vector<SaccItem> recs;
	Structure s_st;
	std::vector<uint64_t> tile_mask; // dense S: filled tile pattern (schur_tile_mask); empty: every tile
	TileDagCost cam_cost[2];               // the model's figures of the natural order / of the order used
	bool cam_dissected = false;            // the camera order is a dissection (arc, arc, separators), not the natural one
	std::vector<int32_t> step_order;       // ... then the step order of the streamed factor on tile_mask (tail_step_order); empty: ascending
};

struct Obs { int32_t lm, pose; int64_t off; };
struct ABlk { int32_t i1, i2; int64_t off; }; // (off: -2 - offset when the block is stored transposed, i.e. its positions are reversed)

// What crosses the phases of schur_plan_host() without being part of its result.
struct PlanScratch {
	std::vector<int32_t> pose_of, lm_of; // per block column: its pose position / its landmark of this shard, or -1
	std::vector<ABlk> ablk;              // the camera-camera blocks, by position
	bool obs_sorted = true;              // the column scan emitted the observations sorted by (landmark, pose)
	std::vector<std::vector<int32_t> > foreign_cols; // per pose i1: poses i2 > i1 co-observing a foreign landmark
	HVec<int32_t> cam_end;               // beside every cam_obs entry: where the observations of its landmark end
	std::vector<int64_t> sblk_beg;       // pair range per S block
	std::vector<int32_t> item_blk, item_beg, item_end, item_slot; // the work items: S block, pair range, partial slot or -1
};

// Phase 1, the partition (also what the tile-mask and camera-order probes start from). Reads the block widths, or with
// mis the graph; fills h.dp, h.dl, h.is_lm, the cameras in their natural order (h.pose_block, w.pose_of, h.nc) and the
// landmarks of this shard (h.lm_block, w.lm_of, h.nl; h.nl_total over all shards).
static void schur_partition(const Structure &st, int shard_rank, int shard_world, bool mis, SchurPlanHost &h, PlanScratch &w)
{
	int dp, dl;
	std::vector<uint8_t> &is_lm = h.is_lm;
	if(mis) {
		SPP_REQUIRE(mis_partition(st, is_lm, &dp), SPP_E_UNSUPPORTED,
			"MIS Schur mode needs a graph of one block width (3 or 6) with at least one edge");
		dl = dp;
	} else {
		SPP_REQUIRE(schur_applicable(st, &dp, &dl), SPP_E_UNSUPPORTED,
			"Schur mode needs exactly two block widths ({6,3} or {3,2}) and a block-diagonal landmark part");
		is_lm.assign(st.nb, 0);
		for(int64_t j = 0; j < st.nb; ++ j)
			is_lm[j] = st.dim[j] == dl;
	}
	h.dp = dp;
	h.dl = dl;

	// ---- guided ordering: stable partition by width (LinearSolver_Schur.cpp:771-838)
	// The cameras keep that (natural) order unless the camera order of a closed loop is accepted (schur_cam_order): from
	// here on a pose is its POSITION, pose_of[] / pose_block[], and everything below goes through the two.
	std::vector<int32_t> &pose_of = w.pose_of, &lm_of = w.lm_of;
	pose_of.assign(st.nb, -1);
	lm_of.assign(st.nb, -1);
	int64_t nc = 0, nl_total = 0, nl = 0;
	for(int64_t j = 0; j < st.nb; ++ j) {
		if(!is_lm[j]) {
			pose_of[j] = (int32_t)nc ++;
			h.pose_block.push_back(j);
		} else {
			// landmark sharding: round-robin over ranks keeps track lengths balanced
			if(nl_total % shard_world == shard_rank) {
				lm_of[j] = (int32_t)nl ++;
				h.lm_block.push_back(j);
			}
			++ nl_total;
		}
	}
	h.nc = nc;
	h.nl = nl;
	h.nl_total = nl_total;
}

// Phase 2, the camera order. Reads the partition; where schur_cam_order() accepts an order, h.pose_block and w.pose_of
// hold it from here on (h.cam_cost: the model's figures of the natural order and of the order used).
static void apply_cam_order(const Structure &st, bool sparse_S, bool mis, SchurPlanHost &h, PlanScratch &w)
{
	const int dp = h.dp;
	const int64_t nc = h.nc;
	const std::vector<uint8_t> &is_lm = h.is_lm;
	std::vector<int32_t> &pose_of = w.pose_of;
	std::vector<int32_t> cam_order;
	if(schur_cam_order(st, is_lm, pose_of, nc, dp, sparse_S, mis, nullptr, cam_order, h.cam_cost)) {
		h.cam_dissected = true;
		const std::vector<int64_t> natural(h.pose_block);
		for(int64_t q = 0; q < nc; ++ q) {
			h.pose_block[q] = natural[cam_order[q]];
			pose_of[h.pose_block[q]] = (int32_t)q;
		}
		if(switches().verbose)
			fprintf(stderr, "[spp] camera order: tiles %lld -> %lld, updates %lld -> %lld, chain %lld -> %lld, model %.0f -> %.0f us\n",
				(long long)h.cam_cost[0].tiles, (long long)h.cam_cost[1].tiles, (long long)h.cam_cost[0].updates,
				(long long)h.cam_cost[1].updates, (long long)h.cam_cost[0].path, (long long)h.cam_cost[1].path,
				h.cam_cost[0].cost_us, h.cam_cost[1].cost_us);
	}
}

// Phase 3, the column scan. Reads the structure through the partition; fills the observations in column order
// (h.obs_lm, h.obs_pose, h.obs_off), w.obs_sorted, the camera-camera blocks w.ablk (h.n_ablk) and h.lm_coff.
static void scan_columns(const Structure &st, SchurPlanHost &h, PlanScratch &w)
{
	const int64_t nl = h.nl;
	const std::vector<uint8_t> &is_lm = h.is_lm;
	const std::vector<int32_t> &pose_of = w.pose_of, &lm_of = w.lm_of;
	// ---- observations: every pose-landmark block, sorted by (landmark, pose). Two passes over ranges of columns on host
	// threads: counts per range, then every range writes its observations / camera-camera blocks at its offset.
	HVec<int64_t> &lm_coff = h.lm_coff;
	lm_coff.assign(nl, -1);
	std::vector<ABlk> &ablk = w.ablk;
	HVec<int32_t> &lm_ptr = h.lm_ptr, &obs_pose = h.obs_pose, &obs_lm = h.obs_lm;
	HVec<int64_t> &obs_off = h.obs_off;
	bool &obs_sorted = w.obs_sorted;
	const int nts = plan_threads(st.nnzb);
	std::vector<int64_t> jcut;
	balanced_cuts(st.col_ptr, nts, jcut);
	{
		std::vector<int64_t> n_obs_t(nts + 1, 0), n_ab_t(nts + 1, 0);
		// what block p of column j is: 0 camera-camera, 1 landmark diagonal, 2 observation (o filled), 3 not of this shard
		auto classify = [&](int64_t j, int64_t p, Obs &o) -> int {
			const int64_t i = st.row_idx[p]; // i <= j
			const bool pi = !is_lm[i], pj = !is_lm[j];
			if(pi && pj)
				return 0;
			if(!pi && !pj)
				return 1;
			if(pi) { // block (pose i, landmark j): dp x dl as stored
				if(lm_of[j] < 0)
					return 3;
				o = {lm_of[j], pose_of[i], st.blk_off[p] << 1};
			} else { // block (landmark i, pose j): stored transposed, dl x dp
				if(lm_of[i] < 0)
					return 3;
				o = {lm_of[i], pose_of[j], (st.blk_off[p] << 1) | 1};
			}
			return 2;
		};
		run_threads(nts, [&](int t) {
			int64_t n_o = 0, n_a = 0;
			Obs o;
			for(int64_t j = jcut[t]; j < jcut[t + 1]; ++ j)
				for(int64_t p = st.col_ptr[j]; p < st.col_ptr[j + 1]; ++ p) {
					const int k = classify(j, p, o);
					n_o += k == 2;
					n_a += k == 0;
				}
			n_obs_t[t + 1] = n_o;
			n_ab_t[t + 1] = n_a;
		});
		for(int t = 0; t < nts; ++ t) {
			n_obs_t[t + 1] += n_obs_t[t];
			n_ab_t[t + 1] += n_ab_t[t];
		}
		const int64_t no_all = n_obs_t[nts];
		SPP_REQUIRE(no_all < (int64_t(1) << 31), SPP_E_UNSUPPORTED, "too many observations for 32-bit obs indices");
		obs_pose.resize(no_all);
		obs_lm.resize(no_all);
		obs_off.resize(no_all);
		ablk.resize(n_ab_t[nts]);
		std::vector<char> sorted_t(nts, 1);
		run_threads(nts, [&](int t) {
			int64_t a = n_obs_t[t], q = n_ab_t[t];
			Obs o, prev = {-1, -1, 0};
			bool sorted = true;
			for(int64_t j = jcut[t]; j < jcut[t + 1]; ++ j)
				for(int64_t p = st.col_ptr[j]; p < st.col_ptr[j + 1]; ++ p) {
					const int k = classify(j, p, o);
					if(k == 0) {
						// i <= j: in the natural order i1 <= i2; a camera order may reverse the two, the block is then the
						// transpose of the upper S block it is added to
						const int32_t pi = pose_of[st.row_idx[p]], pj = pose_of[j];
						ablk[q ++] = pi <= pj ? ABlk{pi, pj, st.blk_off[p]} : ABlk{pj, pi, -2 - st.blk_off[p]};
					}
					else if(k == 1) {
						if(lm_of[j] >= 0)
							lm_coff[lm_of[j]] = st.blk_off[p]; // diagonal C block
					} else if(k == 2) {
						if(o.lm < prev.lm || (o.lm == prev.lm && o.pose < prev.pose))
							sorted = false;
						prev = o;
						obs_lm[a] = o.lm;
						obs_pose[a] = o.pose;
						obs_off[a] = o.off;
						++ a;
					}
				}
			sorted_t[t] = sorted;
		});
		for(int t = 0; t < nts; ++ t)
			obs_sorted = obs_sorted && sorted_t[t];
		for(int t = 1; t < nts && obs_sorted; ++ t) { // across the ranges
			const int64_t a = n_obs_t[t];
			if(a > 0 && a < no_all && (obs_lm[a] < obs_lm[a - 1] || (obs_lm[a] == obs_lm[a - 1] && obs_pose[a] < obs_pose[a - 1])))
				obs_sorted = false;
		}
	}
	h.n_ablk = (int64_t)ablk.size();
	for(int64_t l = 0; l < nl; ++ l)
		SPP_REQUIRE(lm_coff[l] >= 0, SPP_E_BADARG, "landmark without a diagonal block");
}

// Phase 4, the foreign column pattern of a sharded sparse S. Reads the structure through the partition; fills
// w.foreign_cols.
static void foreign_columns(const Structure &st, const SchurPlanHost &h, PlanScratch &w)
{
	const int64_t nc = h.nc;
	const std::vector<uint8_t> &is_lm = h.is_lm;
	const std::vector<int32_t> &pose_of = w.pose_of, &lm_of = w.lm_of;
	std::vector<std::vector<int32_t> > &foreign_cols = w.foreign_cols;
	std::vector<int64_t> lm_gidx(st.nb, -1);
	int64_t g = 0;
	for(int64_t j = 0; j < st.nb; ++ j)
		if(is_lm[j])
			lm_gidx[j] = g ++;
	std::vector<std::vector<int32_t> > poses_of(g);
	for(int64_t j = 0; j < st.nb; ++ j)
		for(int64_t p = st.col_ptr[j]; p < st.col_ptr[j + 1]; ++ p) {
			const int64_t i = st.row_idx[p];
			const bool pi = !is_lm[i], pj = !is_lm[j];
			if(pi && !pj && lm_of[j] < 0)
				poses_of[lm_gidx[j]].push_back(pose_of[i]);
			else if(!pi && pj && lm_of[i] < 0)
				poses_of[lm_gidx[i]].push_back(pose_of[j]);
		}
	foreign_cols.resize(nc);
	for(int64_t l = 0; l < g; ++ l) {
		std::vector<int32_t> &ps = poses_of[l];
		std::sort(ps.begin(), ps.end());
		for(size_t a = 0; a < ps.size(); ++ a)
			for(size_t b = a + 1; b < ps.size(); ++ b)
				foreign_cols[ps[a]].push_back(ps[b]);
	}
	for(int64_t c = 0; c < nc; ++ c) {
		std::sort(foreign_cols[c].begin(), foreign_cols[c].end());
		foreign_cols[c].erase(std::unique(foreign_cols[c].begin(), foreign_cols[c].end()), foreign_cols[c].end());
	}
}

// Phase 5, the order of the observations. Reads w.obs_sorted; leaves h.obs_lm, h.obs_pose, h.obs_off sorted by
// (landmark, pose) and fills h.no and h.lm_ptr.
static void order_observations(SchurPlanHost &h, const PlanScratch &w)
{
	const int64_t nl = h.nl;
	const bool obs_sorted = w.obs_sorted;
	HVec<int32_t> &lm_ptr = h.lm_ptr, &obs_pose = h.obs_pose, &obs_lm = h.obs_lm;
	HVec<int64_t> &obs_off = h.obs_off;
	// (cameras before points, the usual numbering: the column scan above already emits the observations in order)
	const int64_t no = (int64_t)obs_pose.size();
	h.no = no;
	bool lm_sorted = true;
	for(int64_t a = 1; a < no && lm_sorted; ++ a)
		lm_sorted = obs_lm[a - 1] <= obs_lm[a];
	if(!obs_sorted && lm_sorted) {
		// (a camera order: the landmarks still ascend, only the poses inside a landmark's run do not -- short runs, sorted in
		// place on host threads)
		const int nts2 = plan_threads(no);
		run_threads(nts2, [&](int t) {
			int64_t a = no * t / nts2, a1 = no * (t + 1) / nts2;
			while(a > 0 && a < no && obs_lm[a] == obs_lm[a - 1])
				++ a; // (a run belongs to the range it starts in)
			std::vector<std::pair<int32_t, int64_t> > run;
			while(a < a1) {
				int64_t e = a + 1;
				while(e < no && obs_lm[e] == obs_lm[a])
					++ e;
				run.clear();
				for(int64_t q = a; q < e; ++ q)
					run.push_back(std::make_pair(obs_pose[q], obs_off[q]));
				std::sort(run.begin(), run.end());
				for(int64_t q = a; q < e; ++ q) {
					obs_pose[q] = run[q - a].first;
					obs_off[q] = run[q - a].second;
				}
				a = e;
			}
		});
	} else if(!obs_sorted) {
		std::vector<Obs> obs(no);
		for(int64_t a = 0; a < no; ++ a)
			obs[a] = {obs_lm[a], obs_pose[a], obs_off[a]};
		std::sort(obs.begin(), obs.end(), [](const Obs &a, const Obs &b) {
			return a.lm != b.lm ? a.lm < b.lm : a.pose < b.pose; });
		for(int64_t a = 0; a < no; ++ a) {
			obs_lm[a] = obs[a].lm;
			obs_pose[a] = obs[a].pose;
			obs_off[a] = obs[a].off;
		}
	}
	// lm_ptr[l] = number of observations of the landmarks before l: written where the landmark changes
	lm_ptr.resize(nl + 1);
	const int nto = plan_threads(no);
	run_threads(nto, [&](int t) {
		const int64_t a0 = no * t / nto, a1 = no * (t + 1) / nto;
		for(int64_t a = a0; a < a1; ++ a) {
			const int32_t lp = a ? obs_lm[a - 1] : -1, lc = obs_lm[a];
			for(int32_t l = lp + 1; l <= lc; ++ l)
				lm_ptr[l] = (int32_t)a;
		}
	});
	for(int64_t l = (no ? obs_lm[no - 1] : -1) + 1; l <= nl; ++ l)
		lm_ptr[l] = (int32_t)no;
}

// Phase 6, the groups of the back-substitution: consecutive landmarks in groups of at most 256 observations (one workgroup each: the products
// U^T dx of a group stay in LDS, spp_schur.hip backsubst_fused_kernel). Reads h.lm_ptr; fills h.bs_ptr.
static void backsubst_groups(SchurPlanHost &h)
{
	const int64_t nl = h.nl, no = h.no;
	const HVec<int32_t> &lm_ptr = h.lm_ptr;
	const int32_t BS_OBS = 256;
	std::vector<int32_t> &bp = h.bs_ptr;
	bp.clear();
	bp.reserve((size_t)(no / 160 + 2));
	bp.push_back(0);
	int32_t first = 0;
	bool ok = true;
	for(int64_t l = 0; l < nl; ++ l) {
		if(lm_ptr[l + 1] - lm_ptr[l] > BS_OBS) {
			ok = false;
			break;
		}
		if(lm_ptr[l + 1] - lm_ptr[first] > BS_OBS || l - first >= BS_OBS) { // (one lane per observation, then one per landmark)
			bp.push_back((int32_t)l);
			first = (int32_t)l;
		}
	}
	if(ok && nl)
		bp.push_back((int32_t)nl);
	else
		bp.clear();
}

// Phase 7, the per-camera lists. Reads the sorted observations and h.lm_ptr; fills h.cam_ptr, h.cam_obs, w.cam_end
// and h.wpos.
static void camera_lists(SchurPlanHost &h, PlanScratch &w)
{
	const int64_t nc = h.nc, no = h.no;
	const HVec<int32_t> &lm_ptr = h.lm_ptr, &obs_pose = h.obs_pose, &obs_lm = h.obs_lm;
	const int nto = plan_threads(no);
	// ---- per-pose observation lists (ascending landmark = ascending obs index): a counting sort by camera, ranges of
	// observations on host threads (per-range, per-camera counts give every range its place in every camera's list)
	std::vector<int32_t> &cam_ptr = h.cam_ptr;
	HVec<int32_t> &cam_obs = h.cam_obs;
	cam_ptr.assign(nc + 1, 0);
	cam_obs.resize(no);
	// (beside every entry: where the observations of its landmark end -- the pair lists below walk [a, cam_end) per entry and
	// would otherwise chase cam_obs -> obs_lm -> lm_ptr, three dependent cache misses, per observation)
	HVec<int32_t> &cam_end = w.cam_end;
	cam_end.resize(no);
	{
		std::vector<int32_t> cnt((size_t)nto * nc, 0); // [range][camera]
		run_threads(nto, [&](int t) {
			int32_t *c = cnt.data() + (size_t)t * nc;
			for(int64_t a = no * t / nto, a1 = no * (t + 1) / nto; a < a1; ++ a)
				++ c[obs_pose[a]];
		});
		for(int64_t c = 0; c < nc; ++ c) {
			int32_t sum = cam_ptr[c];
			for(int t = 0; t < nto; ++ t) {
				const int32_t v = cnt[(size_t)t * nc + c];
				cnt[(size_t)t * nc + c] = sum; // where range t starts in the list of camera c
				sum += v;
			}
			cam_ptr[c + 1] = sum;
		}
		run_threads(nto, [&](int t) {
			int32_t *fill = cnt.data() + (size_t)t * nc;
			for(int64_t a = no * t / nto, a1 = no * (t + 1) / nto; a < a1; ++ a) {
				const int32_t pos = fill[obs_pose[a]] ++;
				cam_obs[pos] = (int32_t)a;
				cam_end[pos] = lm_ptr[obs_lm[a] + 1];
			}
		});
	}

	// camera-major position of every observation: W, Up, xw are stored in this order, so that the
	// blocks one camera contributes are contiguous (the S accumulation gathers them per camera pair)
	HVec<int32_t> &wpos = h.wpos;
	wpos.resize(no);
	run_threads(nto, [&](int t) {
		for(int64_t q = no * t / nto, q1 = no * (t + 1) / nto; q < q1; ++ q)
			wpos[cam_obs[q]] = (int32_t)q;
	});
}

// Phase 8a, the pair list buffers. Reads h.lm_ptr; fills h.n_pairs, the layout flags h.u_landmark_major and h.factored,
// and sizes h.pair_a and h.pair_b, first touched in order on the threads.
static void alloc_pair_lists(SchurPlanHost &h)
{
	const int64_t nl = h.nl;
	const HVec<int32_t> &lm_ptr = h.lm_ptr;
	std::vector<int64_t> lm_pairs(nl + 1, 0);
	for(int64_t l = 0; l < nl; ++ l) {
		const int64_t k = lm_ptr[l + 1] - lm_ptr[l];
		lm_pairs[l + 1] = lm_pairs[l] + k * (k + 1) / 2;
	}
	const int64_t n_pairs = lm_pairs[nl];
	SPP_REQUIRE(n_pairs < (int64_t(1) << 31), SPP_E_UNSUPPORTED, "too many block products for 32-bit pair indices");
	h.n_pairs = n_pairs;
	h.u_landmark_major = switches().sacc_ulm;
	h.factored = switches().sacc_factored;
	RawBuf<int32_t> &pair_a = h.pair_a, &pair_b = h.pair_b;
	pair_a.resize(n_pairs);
	pair_b.resize(n_pairs);
	{
		// first touch in parallel, in order: the fill below writes ~200 000 interleaved streams, and page faults taken in
		// that order by many threads at once serialize in the kernel
		const int ntt = plan_threads(n_pairs);
		run_threads(ntt, [&](int t) {
			const int64_t b = n_pairs * t / ntt, e = n_pairs * (t + 1) / ntt;
			memset(pair_a.p + b, 0, (size_t)(e - b) * sizeof(int32_t));
			memset(pair_b.p + b, 0, (size_t)(e - b) * sizeof(int32_t));
		});
	}
}

// Phase 8, the S block pattern and the pair lists. Reads the camera lists, w.ablk and w.foreign_cols; fills h.pair_a,
// h.pair_b, the block list h.sblk_i1, h.sblk_i2, h.sblk_aoff (h.n_sblk) and w.sblk_beg.
// Key = (i1 <= i2). The pairs of a block keep the landmark order, which is the
// reference's accumulation order (MultiplyToWith_FBS walks the columns of V = landmarks in ascending order).
// Built row by row of S on host threads (ranges of rows balanced by their pair counts).
static void s_pattern_and_pairs(SchurPlanHost &h, PlanScratch &w, VClock &clk)
{
	const int64_t nc = h.nc, no = h.no, n_pairs = h.n_pairs;
	const HVec<int32_t> &obs_pose = h.obs_pose, &cam_obs = h.cam_obs, &wpos = h.wpos, &cam_end = w.cam_end;
	const std::vector<int32_t> &cam_ptr = h.cam_ptr;
	const std::vector<ABlk> &ablk = w.ablk;
	const std::vector<std::vector<int32_t> > &foreign_cols = w.foreign_cols;
	RawBuf<int32_t> &pair_a = h.pair_a, &pair_b = h.pair_b;
	std::vector<int32_t> &sblk_i1 = h.sblk_i1, &sblk_i2 = h.sblk_i2;
	std::vector<int64_t> &sblk_aoff = h.sblk_aoff;
	std::vector<int64_t> &sblk_beg = w.sblk_beg;
	const int nt = plan_threads(n_pairs);
	const bool ulm = h.u_landmark_major, fact = h.factored;
	// A blocks grouped by row for merging
	std::vector<std::vector<std::pair<int32_t, int64_t> > > a_by_row(nc);
	for(size_t q = 0; q < ablk.size(); ++ q)
		a_by_row[ablk[q].i1].push_back(std::make_pair(ablk[q].i2, ablk[q].off));
	{
		// Row-driven: row i1 of S enumerates its pairs itself -- the observations a of camera i1 (ascending landmark), and
		// for each the observations b >= a of the same landmark (ascending pose = column i2 >= i1) -- once to count its
		// columns and once to write the lists. Nothing is bucketed through memory: the pairs of a row go straight to their
		// place, the observer lists they are enumerated from (11 MB on the Venice shape) stay in cache.
		std::vector<int64_t> row_cnt(nc + 1, 0);
		{
			std::vector<int64_t> ccut;
			balanced_cuts(std::vector<int64_t>(cam_ptr.begin(), cam_ptr.end()), nt, ccut);
			run_threads(nt, [&](int t) {
				for(int64_t c = ccut[t]; c < ccut[t + 1]; ++ c) {
					int64_t sum = 0;
					for(int32_t q = cam_ptr[c]; q < cam_ptr[c + 1]; ++ q)
						sum += cam_end[q] - cam_obs[q]; // pairs (a, b >= a)
					row_cnt[c + 1] = sum;
				}
			});
			for(int64_t c = 0; c < nc; ++ c)
				row_cnt[c + 1] += row_cnt[c];
		}
		clk.lap("pair counts");
		// pass 2: rows are independent (row i1 writes the pairs [row_cnt[i1], row_cnt[i1 + 1]))
		std::vector<int64_t> rcut;
		{
			std::vector<int64_t> w(nc + 1, 0);
			for(int64_t c = 0; c < nc; ++ c)
				w[c + 1] = w[c] + (row_cnt[c + 1] - row_cnt[c]) + (nc - c); // pairs + the scan over the row's columns
			balanced_cuts(w, nt, rcut);
		}
		struct RowOut { std::vector<int32_t> i1, i2; std::vector<int64_t> aoff, beg; };
		std::vector<RowOut> rout(nt);
		run_threads(nt, [&](int t) {
			RowOut &ro = rout[t];
			std::vector<int64_t> col_cnt(nc + 1), a_of_col(nc), start(nc + 1, 0);
			std::vector<char> foreign(nc, 0);
			for(int64_t i1 = rcut[t]; i1 < rcut[t + 1]; ++ i1) {
				const int64_t b0 = row_cnt[i1], b1 = row_cnt[i1 + 1];
				std::fill(col_cnt.begin() + i1, col_cnt.end(), 0);
				std::fill(a_of_col.begin() + i1, a_of_col.end(), -1);
				const int32_t qa0 = cam_ptr[i1], qa1 = cam_ptr[i1 + 1];
				constexpr int32_t AHEAD = 24; // (the observers of the entries ahead: the only access that is not a stream)
				for(int32_t q = qa0; q < qa1; ++ q) {
					if(q + AHEAD < (int32_t)no)
						__builtin_prefetch(&obs_pose[cam_obs[q + AHEAD]]);
					const int32_t a = cam_obs[q], e = cam_end[q];
					for(int32_t b = a; b < e; ++ b)
						++ col_cnt[obs_pose[b] + 1];
				}
				for(size_t q = 0; q < a_by_row[i1].size(); ++ q)
					a_of_col[a_by_row[i1][q].first] = a_by_row[i1][q].second;
				if(!foreign_cols.empty())
					for(size_t q = 0; q < foreign_cols[i1].size(); ++ q)
						foreign[foreign_cols[i1][q]] = 1;
				// blocks of this row, ascending i2
				int64_t out = b0;
				for(int64_t c = i1; c < nc; ++ c) {
					start[c] = out;
					if(col_cnt[c + 1] || a_of_col[c] != -1 || foreign[c]) {
						ro.i1.push_back((int32_t)i1);
						ro.i2.push_back((int32_t)c);
						ro.aoff.push_back(a_of_col[c]);
						ro.beg.push_back(out);
					}
					out += col_cnt[c + 1];
				}
				if(!foreign_cols.empty())
					for(size_t q = 0; q < foreign_cols[i1].size(); ++ q)
						foreign[foreign_cols[i1][q]] = 0;
				// stable: landmark order preserved. The pair lists address W / Up, i.e. camera-major positions (the packed
				// U either camera-major like W, or landmark-major = in observation order: the blocks of one landmark's
				// observers are then one contiguous run, which the blocks of one ROW of S gather together)
				for(int32_t q = qa0; q < qa1; ++ q) {
					if(q + AHEAD < (int32_t)no)
						__builtin_prefetch(&obs_pose[cam_obs[q + AHEAD]]);
					const int32_t a = cam_obs[q], e = cam_end[q];
					const int32_t wa = fact ? a : q; // (the position the pair lists address: observation order in the factored form, else camera-major = wpos[a])
					for(int32_t b = a; b < e; ++ b) {
						int64_t &f = start[obs_pose[b]];
						pair_a[f] = wa;
						pair_b[f] = (ulm || fact) ? b : wpos[b];
						++ f;
					}
				}
				(void)b1;
			}
		});
		clk.lap("pair lists by row");
		size_t nblk = 0;
		for(int t = 0; t < nt; ++ t)
			nblk += rout[t].i1.size();
		sblk_i1.reserve(nblk);
		sblk_i2.reserve(nblk);
		sblk_aoff.reserve(nblk);
		sblk_beg.reserve(nblk + 1);
		for(int t = 0; t < nt; ++ t) {
			sblk_i1.insert(sblk_i1.end(), rout[t].i1.begin(), rout[t].i1.end());
			sblk_i2.insert(sblk_i2.end(), rout[t].i2.begin(), rout[t].i2.end());
			sblk_aoff.insert(sblk_aoff.end(), rout[t].aoff.begin(), rout[t].aoff.end());
			sblk_beg.insert(sblk_beg.end(), rout[t].beg.begin(), rout[t].beg.end());
		}
		sblk_beg.push_back(n_pairs);
	}
	const int64_t n_sblk = (int64_t)sblk_i1.size();
	h.n_sblk = n_sblk;
}

// Phase 9, the sparse reduced system: the written blocks of S as an upper block-CSC structure (columns = i2,
// rows i1 ascending, diagonal last): the block list above is row-major, a counting sort by column
// keeps the rows ascending. Reads the block list; fills h.s_st and h.sblk_voff.
static void sparse_s_structure(SchurPlanHost &h)
{
	const int dp = h.dp;
	const int64_t nc = h.nc, n_sblk = h.n_sblk;
	const std::vector<int32_t> &sblk_i1 = h.sblk_i1, &sblk_i2 = h.sblk_i2;
	Structure &ss = h.s_st;
	ss.nb = nc;
	ss.nnzb = n_sblk;
	ss.dim.assign(nc, dp);
	ss.base.resize(nc + 1);
	for(int64_t c = 0; c <= nc; ++ c)
		ss.base[c] = c * dp;
	ss.n = nc * dp;
	ss.col_ptr.assign(nc + 1, 0);
	for(int64_t b = 0; b < n_sblk; ++ b)
		++ ss.col_ptr[sblk_i2[b] + 1];
	for(int64_t c = 0; c < nc; ++ c)
		ss.col_ptr[c + 1] += ss.col_ptr[c];
	ss.row_idx.resize(n_sblk);
	ss.blk_off.resize(n_sblk);
	std::vector<int64_t> fill(ss.col_ptr.begin(), ss.col_ptr.end() - 1);
	h.sblk_voff.resize(n_sblk);
	for(int64_t b = 0; b < n_sblk; ++ b) {
		const int64_t q = fill[sblk_i2[b]] ++;
		ss.row_idx[q] = sblk_i1[b];
		ss.blk_off[q] = q * dp * dp;
		h.sblk_voff[b] = q * dp * dp;
	}
	ss.nvals = n_sblk * dp * dp;
	for(int64_t c = 0; c < nc; ++ c)
		SPP_REQUIRE(ss.col_ptr[c + 1] > ss.col_ptr[c] && ss.row_idx[ss.col_ptr[c + 1] - 1] == c, SPP_E_BADARG,
			"a pose without any diagonal contribution: the reduced system is singular");
}

// Phase 10, the work items: chunks of at most PAIR_CHUNK pairs, ordered tile by tile and dealt to the XCDs by work.
// Reads the block list and w.sblk_beg; fills w.item_* (in execution order), h.multi_blk, h.multi_ptr, h.n_slots,
// h.n_items, h.n_multi, h.xb and h.xcd_max_items.
static void work_items(SchurPlanHost &h, PlanScratch &w)
{
	const int64_t nc = h.nc, n_sblk = h.n_sblk;
	const std::vector<int32_t> &sblk_i1 = h.sblk_i1, &sblk_i2 = h.sblk_i2;
	const std::vector<int64_t> &sblk_beg = w.sblk_beg;
	std::vector<int32_t> &item_blk = w.item_blk, &item_beg = w.item_beg, &item_end = w.item_end, &item_slot = w.item_slot;
	std::vector<int32_t> &multi_blk = h.multi_blk, &multi_ptr = h.multi_ptr;
	int32_t n_slots = 0;
	for(int64_t b = 0; b < n_sblk; ++ b) {
		const int64_t beg = sblk_beg[b], end = sblk_beg[b + 1];
		const int64_t nchunk = std::max<int64_t>(1, (end - beg + PAIR_CHUNK - 1) / PAIR_CHUNK);
		if(nchunk > 1) {
			multi_blk.push_back((int32_t)b);
			multi_ptr.push_back(n_slots);
		}
		for(int64_t c = 0; c < nchunk; ++ c) {
			item_blk.push_back((int32_t)b);
			item_beg.push_back((int32_t)(beg + c * PAIR_CHUNK));
			item_end.push_back((int32_t)std::min<int64_t>(end, beg + (c + 1) * PAIR_CHUNK));
			item_slot.push_back(nchunk > 1 ? n_slots ++ : -1);
		}
	}
	multi_ptr.push_back(n_slots);
	h.n_slots = n_slots;
	// Item order = execution order. Blocks are visited tile by tile (SACC_TILE x SACC_TILE cameras):
	// the W segments of the tile's row cameras and the U segments of its column cameras (~0.5 MB each
	// on Venice) then stay in the L2 of the XCD that works through the tile (the kernel hands each XCD
	// one contiguous range of items).
	bool interleave = false;
	std::vector<int32_t> xb_il;
	{
		const int64_t tb_env = switches().sacc_tile, tbc_env = switches().sacc_tile_cols; // (-2: as the tile's side)
		const int64_t TB = tb_env, TBC = (tbc_env == -2) ? TB : (tbc_env <= 0 ? nc : tbc_env), ntile = (nc + TBC - 1) / TBC;
		std::vector<int32_t> perm(item_blk.size());
		for(size_t q = 0; q < perm.size(); ++ q)
			perm[q] = (int32_t)q;
		interleave = switches().sacc_xcd != 0;
		std::vector<int64_t> tile_of_item(item_blk.size());
		for(size_t q = 0; q < tile_of_item.size(); ++ q)
			tile_of_item[q] = (sblk_i1[item_blk[q]] / TB) * ntile + sblk_i2[item_blk[q]] / TBC;
		auto tile_of = [&](int32_t q) { return tile_of_item[q]; };
		// (stable sorts by small keys: counting sorts -- two comparison sorts of the 180 000 items of the Venice shape were
		// 15 ms of the plan)
		auto stable_by_key = [&](std::vector<int32_t> &pm, int64_t n_keys, auto key_of) {
			if(n_keys > 8 * (int64_t)pm.size() + 1024) {
				std::stable_sort(pm.begin(), pm.end(), [&](int32_t x, int32_t y) { return key_of(x) < key_of(y); });
				return;
			}
			std::vector<int32_t> start((size_t)n_keys + 1, 0), out(pm.size());
			for(size_t q = 0; q < pm.size(); ++ q)
				++ start[key_of(pm[q]) + 1];
			for(int64_t k = 0; k < n_keys; ++ k)
				start[k + 1] += start[k];
			for(size_t q = 0; q < pm.size(); ++ q)
				out[start[key_of(pm[q])] ++] = pm[q];
			pm.swap(out);
		};
		stable_by_key(perm, ((nc + TB - 1) / TB) * ntile, tile_of);
		if(interleave) {
			// All eight XCDs work in the same neighbourhood of S: consecutive tiles (in tile-row-major order) go to
			// consecutive XCDs. A tile's camera segments still meet in ONE L2, and the blocks every XCD re-reads
			// within a band of S now share one working set in the memory-side cache (256 MB) instead of eight.
			// The deal is by WORK, not by count: the next tile goes to the XCD with the least work so far (a wave spends a
			// fixed cost per item plus one gather round per 64 pairs) -- on a banded S every eighth tile can be a diagonal
			// one, ten times as heavy as its neighbours (config 5 shape: 2.65 ms dealt by count, 1.5 ms by work).
			std::vector<int32_t> xcd_of(perm.size());
			int64_t load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
			for(size_t q = 0; q < perm.size();) {
				const int64_t t = tile_of(perm[q]);
				size_t e = q;
				int64_t cost = 0;
				for(; e < perm.size() && tile_of(perm[e]) == t; ++ e)
					cost += 2 + (item_end[perm[e]] - item_beg[perm[e]] + 63) / 64;
				int x = 0;
				for(int y = 1; y < 8; ++ y)
					if(load[y] < load[x])
						x = y;
				load[x] += cost;
				for(size_t i = q; i < e; ++ i)
					xcd_of[perm[i]] = x;
				q = e;
			}
			stable_by_key(perm, 8, [&](int32_t x) { return (int64_t)xcd_of[x]; });
			xb_il.assign(9, 0);
			for(size_t q = 0; q < perm.size(); ++ q)
				++ xb_il[xcd_of[q] + 1];
			for(int x = 0; x < 8; ++ x)
				xb_il[x + 1] += xb_il[x];
		}
		std::vector<int32_t> t_blk(perm.size()), t_beg(perm.size()), t_end(perm.size()), t_slot(perm.size());
		for(size_t q = 0; q < perm.size(); ++ q) {
			t_blk[q] = item_blk[perm[q]];
			t_beg[q] = item_beg[perm[q]];
			t_end[q] = item_end[perm[q]];
			t_slot[q] = item_slot[perm[q]];
		}
		item_blk.swap(t_blk); item_beg.swap(t_beg); item_end.swap(t_end); item_slot.swap(t_slot);
	}
	h.n_items = (int64_t)item_blk.size();
	// eight item ranges (one per XCD). Contiguous ranges: of equal WORK -- a wave spends a fixed cost per item plus
	// one gather round per 64 pairs; equal item counts would leave the last range ~45 % heavier
	{
		std::vector<int32_t> &xb = h.xb;
		xb.assign(9, 0);
		if(interleave)
			xb = xb_il;
		else {
			std::vector<int64_t> cost(h.n_items + 1, 0);
			for(int64_t q = 0; q < h.n_items; ++ q)
				cost[q + 1] = cost[q] + 2 + (item_end[q] - item_beg[q] + 63) / 64;
			for(int x = 1; x < 8; ++ x)
				xb[x] = (int32_t)(std::lower_bound(cost.begin(), cost.end(), cost[h.n_items] * x / 8) - cost.begin());
			xb[8] = (int32_t)h.n_items;
		}
		h.xcd_max_items = 0;
		for(int x = 0; x < 8; ++ x) {
			xb[x + 1] = std::max(xb[x + 1], xb[x]);
			h.xcd_max_items = std::max(h.xcd_max_items, xb[x + 1] - xb[x]);
		}
	}
	h.n_multi = (int64_t)multi_blk.size();
}

// Phase 11a, the rhs offsets. Reads h.pose_block and h.lm_block; fills h.pose_rbase and h.lm_rbase.
static void rhs_offsets(const Structure &st, SchurPlanHost &h)
{
	const int64_t nc = h.nc, nl = h.nl;
	h.pose_rbase.resize(nc);
	h.lm_rbase.resize(nl);
	for(int64_t c = 0; c < nc; ++ c)
		h.pose_rbase[c] = st.base[h.pose_block[c]];
	for(int64_t l = 0; l < nl; ++ l)
		h.lm_rbase[l] = st.base[h.lm_block[l]];
}

// Phase 11, the item records. Reads w.item_* and the block list; fills h.recs:
// self-contained item records (one 32-byte load per item in the kernel)
static void item_records(bool add_A, bool sparse_S, SchurPlanHost &h, const PlanScratch &w)
{
	const int dp = h.dp;
	const std::vector<int32_t> &sblk_i1 = h.sblk_i1, &sblk_i2 = h.sblk_i2;
	const std::vector<int64_t> &sblk_aoff = h.sblk_aoff;
	const std::vector<int32_t> &item_blk = w.item_blk, &item_beg = w.item_beg, &item_end = w.item_end, &item_slot = w.item_slot;
	h.recs.resize(item_blk.size());
	for(size_t q = 0; q < h.recs.size(); ++ q) {
		const int32_t b = item_blk[q];
		SaccItem &r = h.recs[q];
		r.beg = item_beg[q];
		r.end = item_end[q];
		r.a_tr = 0;
		r.aoff = -1;
		if(item_slot[q] >= 0) { // split block: s_multi_kernel sums the slots and adds A
			r.kind = 2;
			r.dst = (int64_t)item_slot[q] * dp * dp;
		} else {
			r.aoff = add_A ? sblk_aoff[b] : -1;
			if(r.aoff < -1) { // stored transposed
				r.aoff = -2 - r.aoff;
				r.a_tr = 1;
			}
			if(sparse_S) {
				r.kind = 1;
				r.dst = h.sblk_voff[b];
			} else {
				r.kind = 0;
				r.dst = (int64_t)sblk_i1[b] * dp + (int64_t)sblk_i2[b] * dp * h.ld;
			}
		}
	}
}

// The plan: the phases above in their order, lap by lap (SPP_VERBOSE).
static void schur_plan_host(const Structure &st, int shard_rank, int shard_world, bool sparse_S, bool mis, SchurPlanHost &h)
{
	VClock clk("schur plan");
	PlanScratch w;
	schur_partition(st, shard_rank, shard_world, mis, h, w);
	apply_cam_order(st, sparse_S, mis, h, w);
	clk.lap("camera order");
	h.n_red = h.nc * h.dp;
	h.ld = ((h.n_red + 1 + DENSE_NB - 1) / DENSE_NB) * DENSE_NB; // at least one padding column (rhs)
	SPP_REQUIRE(sparse_S || h.ld <= 65536, SPP_E_UNSUPPORTED,
		"reduced camera system too large for the dense path (use SPP_MODE_SCHUR_SPARSE)");
	if(!sparse_S)
		schur_tile_mask(st, h.is_lm, w.pose_of, h.dp, h.n_red, h.tile_mask);
	// The step order of the streamed factor: only under a dissected camera order, whose arcs emit their row tiles side by
	// side (every other order keeps its steps ascending, bit for bit as before). From the mask over ALL shards and from
	// nothing a run-time switch of the factor's scheduling changes: every rank, and SPP_TAIL_MASK = 0 / 1, get the same one.
	if(h.cam_dissected && !h.tile_mask.empty() && switches().tail_step_order) {
		tail_step_order(h.tile_mask, h.step_order);
		bool identity = true;
		for(size_t q = 0; q < h.step_order.size(); ++ q)
			identity = identity && h.step_order[q] == (int32_t)q;
		if(identity)
			h.step_order.clear();
	}
	scan_columns(st, h, w);
	clk.lap("partition + observation scan");
	// Sharded + sparse reduced system: every rank must hold the SAME block structure of S (the union
	// over all landmarks), or the all-reduce of the value arrays would add unrelated blocks. The pattern
	// of the landmarks this rank does not own is collected here (pose lists per foreign landmark).
	if(sparse_S && shard_world > 1)
		foreign_columns(st, h, w);
	order_observations(h, w);
	backsubst_groups(h);
	camera_lists(h, w);
	clk.lap("observation / camera lists");
	alloc_pair_lists(h);
	clk.lap("pair list buffers");
	s_pattern_and_pairs(h, w, clk); // (laps "pair counts" and "pair lists by row" inside)
	if(sparse_S)
		sparse_s_structure(h);
	clk.lap("block lists");
	work_items(h, w);
	rhs_offsets(st, h);
	clk.lap("work items");
	item_records(shard_rank == 0, sparse_S, h, w); // (rank 0 adds A)
	clk.lap("item records");
}

void build_schur_plan(spp_ctx *ctx, bool sparse_S, bool mis)
{
	const Structure &st = ctx->st;
	SchurPlan &sp = ctx->schur;
	sp.release_all();
	sp.sparse_S = sparse_S;
	hipStream_t s = ctx->stream;
	VClock clk0("schur plan (device)");
	std::unique_ptr<SchurPlanHost> hp(new SchurPlanHost);
	SchurPlanHost &h = *hp;
	clk0.lap("old plan released");
	schur_plan_host(st, ctx->shard_rank, ctx->shard_world, sparse_S, mis, h);
	VClock clk("schur plan (device)");
	const int dp = h.dp, dl = h.dl;
	const int64_t nl = h.nl, no = h.no;
	static_cast<SchurDims &>(sp) = h;
	sp.pose_block.swap(h.pose_block);
	sp.lm_block.swap(h.lm_block);
	sp.is_lm.swap(h.is_lm);
	sp.add_A = (ctx->shard_rank == 0);
	sp.tile_mask.swap(h.tile_mask);
	sp.step_order.swap(h.step_order);
	if(sparse_S) {
		sp.s_st = h.s_st;
		sp.sblk_voff.upload(h.sblk_voff, s);
	}

	// ---- upload
	sp.xcd_beg.upload(h.xb, s);
	sp.lm_ptr.upload(h.lm_ptr, s);
	sp.n_bs = h.bs_ptr.empty() ? 0 : (int64_t)h.bs_ptr.size() - 1;
	sp.bs_ptr.upload(h.bs_ptr, s);
	sp.lm_coff.upload(h.lm_coff, s);
	sp.lm_rbase.upload(h.lm_rbase, s);
	sp.obs_pose.upload(h.obs_pose, s);
	sp.obs_lm.upload(h.obs_lm, s);
	sp.obs_off.upload(h.obs_off, s);
	sp.pose_rbase.upload(h.pose_rbase, s);
	sp.cam_ptr.upload(h.cam_ptr, s);
	sp.cam_obs.upload(h.cam_obs, s);
	sp.items.upload(h.recs, s);
	sp.obs_wpos.upload(h.wpos, s);
	sp.sblk_i1.upload(h.sblk_i1, s);
	sp.sblk_i2.upload(h.sblk_i2, s);
	sp.sblk_aoff.upload(h.sblk_aoff, s);
	sp.pair_a.reserve(std::max<size_t>(1, h.pair_a.size()));
	sp.pair_b.reserve(std::max<size_t>(1, h.pair_b.size()));
	if(h.pair_a.size()) {
		SPP_HIP_CHECK(hipMemcpyAsync(sp.pair_a.p, h.pair_a.p, h.pair_a.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
		SPP_HIP_CHECK(hipMemcpyAsync(sp.pair_b.p, h.pair_b.p, h.pair_b.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
	}
	sp.multi_blk.upload(h.multi_blk, s);
	sp.multi_ptr.upload(h.multi_ptr, s);
	clk.lap("uploads enqueued");
	sp.cinv.reserve((size_t)std::max<int64_t>(1, nl) * dl * dl);
	sp.W.reserve((size_t)std::max<int64_t>(1, no) * dp * dl);
	if(sp.factored)
		sp.lfac.reserve((size_t)std::max<int64_t>(1, nl) * dl * dl);
	else
		sp.Up.reserve((size_t)std::max<int64_t>(1, no) * dp * dl);
	sp.xw.reserve((size_t)std::max<int64_t>(1, no) * dp);
	sp.partial.reserve((size_t)std::max<int32_t>(1, h.n_slots) * dp * dp);
	clk.lap("workspaces allocated");
	SPP_HIP_CHECK(hipStreamSynchronize(s)); // host vectors die here
	clk.lap("uploads done");

	if(!sparse_S)
		dense_reserve(ctx, (sp.n_red + DENSE_NB - 1) / DENSE_NB);
	clk.lap("dense workspaces");

	// ---- accounting (SURVEY 8d "Schur" + "Dense reduced solve")
	const double n = (double)sp.n_red;
	ctx->factor_flops = (int64_t)(n * n * n / 3.0 + 2.0 * n * n);
	ctx->factor_nnz = sp.ld * sp.ld;
	const int64_t blk_pl = 8 * dp * dl, blk_pp = 8 * dp * dp, blk_ll = 8 * dl * dl;
	ctx->solve_bytes = blk_pl * no + blk_ll * nl + blk_pp * h.n_ablk + 8 * st.n /* read */
		+ blk_pp * sp.n_sblk + 8 * st.n /* write S, solution */
		+ 8 * sp.n_red * sp.n_red /* dense factor touched once in place */;
	// the host image (pair lists, observation lists: ~250 MB on a Venice-sized problem, 8 ms to unmap) is released beside
	// the caller
	if(ctx->plan_trash.joinable())
		ctx->plan_trash.join();
	{
		SchurPlanHost *raw = hp.release();
		try {
			ctx->plan_trash = std::thread([raw]() { delete raw; });
		} catch(...) {
			delete raw;
		}
	}
	clk.lap("host plan handed to the releasing thread");
}

// host-only: the symbolic Schur plan of a structure, timed; out[0..8] = nc, nl, no, n_pairs, n_sblk, n_items, n_multi,
// a checksum of the pair lists, block list, item records and XCD ranges, and a checksum of every list and scalar that
// build_schur_plan() uploads or keeps (tests/test_schur_plan_host.py holds recorded values of both); mis: the MIS cut of
// a graph of one block width instead of the guided one
double schur_plan_host_probe(const Structure &st, int shard_rank, int shard_world, bool sparse_S, bool mis, int64_t *out)
{
	const auto t0 = std::chrono::steady_clock::now();
	SchurPlanHost h;
	schur_plan_host(st, shard_rank, shard_world, sparse_S || mis, mis, h);
	const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
	uint64_t sum = 1469598103934665603ull;
	auto mix = [&](uint64_t v) { sum = (sum ^ v) * 1099511628211ull; };
	for(size_t q = 0; q < h.pair_a.size(); ++ q)
		mix(((uint64_t)(uint32_t)h.pair_a[q] << 32) | (uint32_t)h.pair_b[q]);
	for(size_t q = 0; q < h.sblk_i1.size(); ++ q) {
		mix(((uint64_t)(uint32_t)h.sblk_i1[q] << 32) | (uint32_t)h.sblk_i2[q]);
		mix((uint64_t)h.sblk_aoff[q]);
	}
	for(size_t q = 0; q < h.recs.size(); ++ q) {
		mix(((uint64_t)(uint32_t)h.recs[q].beg << 32) | (uint32_t)h.recs[q].end);
		mix((uint64_t)h.recs[q].dst);
		mix((uint64_t)h.recs[q].aoff + (uint64_t)h.recs[q].kind + ((uint64_t)h.recs[q].a_tr << 8)); // (a_tr = 0 in the natural order)
	}
	for(size_t q = 0; q < h.xb.size(); ++ q)
		mix((uint64_t)h.xb[q]);
	// out[8]: everything build_schur_plan() uploads or keeps -- out[7], the scalars, and every list led by its length
	uint64_t all = 1469598103934665603ull;
	auto mix_all = [&](uint64_t v) { all = (all ^ v) * 1099511628211ull; };
	auto mix_list = [&](const auto &v) {
		mix_all((uint64_t)v.size());
		for(size_t q = 0; q < v.size(); ++ q)
			mix_all((uint64_t)(int64_t)v[q]);
	};
	mix_all(sum);
	for(int64_t v : {(int64_t)h.dp, (int64_t)h.dl, h.nc, h.nl, h.nl_total, h.no, h.n_red, h.ld, h.n_sblk, h.n_pairs, h.n_items, h.n_multi,
		h.n_ablk, (int64_t)h.n_slots, (int64_t)h.xcd_max_items, (int64_t)h.u_landmark_major, (int64_t)h.factored})
		mix_all((uint64_t)v);
	mix_list(h.pose_block); mix_list(h.lm_block); mix_list(h.is_lm); mix_list(h.tile_mask);
	mix_list(h.lm_ptr); mix_list(h.bs_ptr); mix_list(h.lm_coff); mix_list(h.lm_rbase);
	mix_list(h.obs_pose); mix_list(h.obs_lm); mix_list(h.obs_off); mix_list(h.pose_rbase);
	mix_list(h.cam_ptr); mix_list(h.cam_obs); mix_list(h.wpos);
	mix_list(h.multi_blk); mix_list(h.multi_ptr); mix_list(h.sblk_voff);
	for(int64_t v : {h.s_st.nb, h.s_st.n, h.s_st.nnzb, h.s_st.nvals})
		mix_all((uint64_t)v);
	mix_list(h.s_st.col_ptr); mix_list(h.s_st.row_idx); mix_list(h.s_st.blk_off); mix_list(h.s_st.base); mix_list(h.s_st.dim);
	mix_all((uint64_t)h.recs.size());
	for(size_t q = 0; q < h.recs.size(); ++ q) // (field by field: out[7] adds three of them up)
		for(int64_t v : {(int64_t)h.recs[q].kind, (int64_t)h.recs[q].a_tr, h.recs[q].dst, h.recs[q].aoff})
			mix_all((uint64_t)v);
	out[0] = h.nc; out[1] = h.nl; out[2] = h.no; out[3] = h.n_pairs; out[4] = h.n_sblk; out[5] = h.n_items; out[6] = h.n_multi;
	out[7] = (int64_t)sum;
	out[8] = (int64_t)all;
	return sec;
}

// host-only: the filled tile mask the dense Schur plan of a structure carries in the natural camera order (every shard's
// is the same)
void schur_tile_mask_host_probe(const Structure &st, std::vector<uint64_t> &words)
{
	SchurPlanHost h;
	PlanScratch w;
	schur_partition(st, 0, 1, false, h, w);
	schur_tile_mask(st, h.is_lm, w.pose_of, h.dp, h.nc * h.dp, words);
}

bool schur_step_order_host_probe(const Structure &st, int shard_rank, int shard_world, bool sparse_S, bool mis, std::vector<int32_t> &step_order)
{
	SchurPlanHost h;
	schur_plan_host(st, shard_rank, shard_world, sparse_S || mis, mis, h);
	const bool carried = !h.step_order.empty();
	step_order = h.step_order;
	if(!carried) {
		step_order.resize(h.tile_mask.size());
		for(size_t q = 0; q < step_order.size(); ++ q)
			step_order[q] = (int32_t)q;
	}
	return carried;
}

bool schur_cam_order_host_probe(const Structure &st, int shard_rank, int shard_world, bool sparse_S, bool mis, const int64_t *order_in,
	std::vector<int32_t> &cam_order, TileDagCost cost[2])
{
	if(!order_in) {
		// the order of the PLAN of this shard, read back from its pose_block[] (not a second evaluation of the rule)
		SchurPlanHost h;
		schur_plan_host(st, shard_rank, shard_world, sparse_S || mis, mis, h);
		std::vector<int32_t> cam_of(st.nb, -1);
		int32_t nc = 0;
		for(int64_t j = 0; j < st.nb; ++ j)
			if(!h.is_lm[j])
				cam_of[j] = nc ++;
		cam_order.resize((size_t)nc);
		bool used = false;
		for(int32_t q = 0; q < nc; ++ q) {
			cam_order[q] = cam_of[h.pose_block[q]];
			used = used || cam_order[q] != q;
		}
		cost[0] = h.cam_cost[0];
		cost[1] = h.cam_cost[1];
		return used;
	}
	SPP_REQUIRE(!sparse_S && !mis, SPP_E_UNSUPPORTED,
		"the model of a given camera order needs the dense guided Schur mode ({6,3} or {3,2} block widths)");
	SchurPlanHost h;
	PlanScratch w;
	schur_partition(st, 0, 1, false, h, w);
	return schur_cam_order(st, h.is_lm, w.pose_of, h.nc, h.dp, false, false, order_in, cam_order, cost);
}

} // namespace spp
