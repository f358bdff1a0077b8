// spp_switches.h -- every run-time switch of libspp_hip.so: one field each, parsed from the environment in ONE place.
//
// The switches are read once per process, on the first call of switches(), and never again: a value changed in the
// environment of a live process afterwards has no effect (before this header some of them -- the orderings, the team
// shape, the S accumulation's layout, SPP_VERBOSE -- were re-read by every analysis). Nothing in tests/, tools/ or
// bench.py relies on a re-read: every variant test starts a child process with the switch in its environment, and
// tools/sparse_stats.py sets SPP_VERBOSE before it imports the library. tools/README.md lists the same names for users;
// tests/test_switches_doc.py keeps that table and the string literals of this file equal, and getenv out of the rest
// of csrc/. (Not the library's: SPP_ADAPTER_FLATTEN_THREADS of the header-only include/spp_adapter.h, and the Python
// side's SPP_LIB / SPP_EXTRA_DEFS.)
#pragma once

#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>

namespace spp {

// device-side waits are bounded in ticks of the 100 MHz wall clock
constexpr long long WAIT_TICKS_PER_MS = 100000;
constexpr long long WAIT_TICKS_DEFAULT = 500 * WAIT_TICKS_PER_MS; // 0.5 s: the bound of every wait that has no switch of its own

enum Ordering { ORDERING_AUTO, ORDERING_AMD, ORDERING_ND };
constexpr int MID_FRONT_MAX = 640; // largest padded height the one-workgroup in-place (HBM image) kernel of the sparse path is built for

struct Switches {
	// ---- all paths
	bool verbose;             // SPP_VERBOSE (off; set to anything = on): analysis statistics and set-up laps on stderr
	int plan_threads;         // SPP_PLAN_THREADS (0 = automatic: up to 16; otherwise >= 1): host threads of the symbolic phases
	int64_t plan_min_work;    // SPP_PLAN_MIN_WORK (2^18, >= 1): entries below which a symbolic pass stays on one thread (tests: 1 cuts even the smallest problem among the threads)

	// ---- dense factor (spp_dense.hip)
	int dense_sched;          // SPP_DENSE_SCHED (1): 0: cross-stream events (round 1), 1: device flags
	int fused;                // SPP_FUSED (1): 0: tile row / update, potrf_diag and panel solve as three launches (round 1)
	int aux_reserve_cus;      // SPP_AUX_RESERVE_CUS (32): CUs the bulk stream's mask leaves to the chain (<= 0: no mask, a low-priority stream)
	int tile_444;             // SPP_TILE_444 (0): whole 128 x 128 tiles: 0 register-staged 16x16x4 tile (rounds 1-2), 1 LDS-DMA 16x16x4 tile, 2 LDS-DMA 4x4x4_4b tile
	int dense_la;             // SPP_DENSE_LA (0): 1: the lookahead schedule (spp_dense_la.h); 0: the two-stream schedule of rounds 1-2
	int la_chain_mask;        // SPP_LA_CHAIN_MASK (1): 0: the lookahead schedule's chain kernel on an unmasked stream
	int la_g2;                // SPP_LA_G2 (0 = all the reservation leaves): workgroups of the chain kernel's panel group
	int la_bulk_acquire;      // SPP_LA_BULK_ACQUIRE (1): 1: the bulk workgroups of the lookahead schedule run an agent-scope acquire behind their poll
	int64_t la_slots;         // SPP_LA_SLOTS (0 = 512): the first multiple of this many tiles of a bulk launch go whole, the rest in quarters
	int la_trace;             // SPP_LA_TRACE (off): n: the n-th factorization prints when its diagonal blocks started / ended
	int tail_rows;            // SPP_TAIL_ROWS (44); 0 when SPP_DENSE_TAIL=0 (1: the streamed tail; 0: the per-step single-stream tail of round 2): tile rows from which on the factorization is streamed
	int tail_mask;            // SPP_TAIL_MASK (1): 0: every tile, whatever structure the caller knows (A/B timing, tests)
	double tail_order_beta;   // SPP_TAIL_ORDER_BETA (0): the streamed launch's workgroup order key i + beta j (0 = row by row)
	int tail_early;           // SPP_TAIL_EARLY (1): with a tile mask, the trailing tile rows whose every tile lags go to the front of the streamed launch's workgroup order (tail_order_table); 0: the sorted order alone
	int tail_step_order;      // SPP_TAIL_STEP_ORDER (1): under a dissected camera order the tiles of the streamed launch apply their steps by the depth of the step's diagonal tile (the arcs' steps interleaved as they are emitted, tail_step_order); 0: ascending
	int tail_early_lead;      // SPP_TAIL_EARLY_LEAD (1): under a step order, a trailing run of lagging tile rows that is too large to be seated whole has its leading rows seated first (tail_order_table); 0: nothing of it. The table alone changes: same bits either way
	long long tail_timeout_ticks; // SPP_TAIL_TIMEOUT_TICKS (5e7 = 0.5 s): bound of a wait of the streamed launch (tests: a tiny value forces the timeout and the per-step fallback)
	int tail_trace;           // SPP_TAIL_TRACE (off): n: the n-th launch prints per tile row when its diagonal tile had all updates, was factored, and when the first panel tile started / ended
	int trsv_chain;           // SPP_TRSV_CHAIN (2): 2: the chain inside one workgroup, 1: a workgroup per hop (round 2), 0: a launch per hop (round 1)
	int trsv_mform;           // SPP_TRSV_MFORM (1): 0: the chain applies R_{b, b+1} and Tinv_b itself (two tiles per hop)
	long long chain_timeout_ticks; // SPP_CHAIN_TIMEOUT_TICKS (5e7 = 0.5 s): bound of a wait inside the backward-substitution chain kernels (tests: a tiny value forces the timeout and the fallback to a launch per block row)
	int trsm_fused;           // SPP_TRSM_FUSED (1): multi-column solves on the kept factor: one launch per step, every updating workgroup forms X_J itself; 0: two launches per step (X_J stored, then the updates read it). Same bits either way

	// ---- Schur complement (spp_schur_plan.cpp, spp_schur.hip)
	bool sacc_ulm;            // SPP_SACC_ULM (1): (unfactored form) packed U landmark-major; 0: camera-major like W
	bool sacc_factored;       // SPP_SACC_FACTORED (1): 0: two packed blocks per observation (W and U), as in rounds 1-2
	int64_t sacc_tile;        // SPP_SACC_TILE (4, >= 1): cameras per side of an item tile (1 = plain row-major block order)
	int64_t sacc_tile_cols;   // SPP_SACC_TILE_COLS (-2 = as SPP_SACC_TILE): cameras per tile along a row of S (<= 0: the whole row)
	int sacc_xcd;             // SPP_SACC_XCD (1): 1: tiles dealt round-robin to the XCDs, 0: one contiguous range per XCD
	int sacc_chunk;           // SPP_SACC_CHUNK (1): items per wave (<= 0 = one persistent set of workgroups). Measured on the Venice shape: 1 -> 0.86 ms, 4...16 -> 0.98 ms, persistent 1.5 ms: the hardware's dynamic dispatch of one-item waves balances the uneven items (1 ... 2048 pairs) better than the software pipeline across items hides latency
	int schur_cam_order;      // SPP_SCHUR_CAM_ORDER (1): dense S with a tile mask: the cameras of a closed loop are ordered arc, arc, separators (tile-aligned dissection, schur_cam_order) when the cost model of the streamed factor gains 10 %; 0: the natural order always
	int backsubst_fused;      // SPP_BACKSUBST_FUSED (1): 0: the products U^T dx through memory, two launches (rounds 1-3)
	int schur_side;           // SPP_SCHUR_SIDE (1): the reduced right-hand side, the padding of S and the status reset run on a side stream beside the S accumulation, from SCHUR_SIDE_MIN_OBS observations on; 0: the serial order on the one stream; 2: the side stream whatever the size (tests)
	int solve_async;          // SPP_SOLVE_ASYNC (1): dense reduced system: the factor's status travels to the host on the side stream while the triangular solves and the back-substitution run, and the solve returns once the status is known, its result ordered on the ctx stream (never under stream capture or with profiling on); 0: the status is fetched behind the back-substitution and the call drains the stream
	int lm_stream;            // SPP_LM_STREAM (1): (factored form, 6 x 3 blocks) the landmark-side kernels fetch U cooperatively in 16-byte pieces, xw in observation order, the fused back-substitution with the next group's fetch in flight; 2: the same with xw camera-major in 16-byte pieces (measured slower: Venice step 2.675 against 2.618 ms); 0: one lane per block (rounds 3-7)

	// ---- sparse path (spp_sparse.hip)
	int mid_front_max;        // SPP_MID_FRONT_MAX (320, clamped to 128 .. MID_FRONT_MAX): fronts above this padded height go to the dense MFMA kernels (with the single-stream dense steps 320 measured best on sphere2500, neutral on the other sparse workloads)
	Ordering ordering;        // SPP_ORDERING (auto): "nd" forces nested dissection, any other value ("amd") minimum degree
	int64_t amalg_small;      // SPP_AMALG_SMALL (32): merged pivot widths up to this are always accepted
	double amalg_zeros;       // SPP_AMALG_ZEROS (0.12): explicit zeros a merged supernode may hold, as a fraction of its panel
	int64_t amalg_relax_h;    // SPP_AMALG_RELAX_H (96): merged fronts up to this height get the looser bound
	double amalg_zeros_small; // SPP_AMALG_ZEROS_SMALL (0.2): that looser bound
	bool sparse_teams;        // SPP_SPARSE_TEAMS (1): big fronts inside the dependency-driven launch by teams of workgroups; 0: through the host-driven dense factor
	int sparse_team_max;      // SPP_SPARSE_TEAM_MAX (40, clamped to 1 .. 64; the device's half CU count bounds it further): largest team
	int sparse_team_cols;     // SPP_SPARSE_TEAM_COLS (16, clamped to 8 .. 256): columns of the padded front per member
	int sparse_dag;           // SPP_SPARSE_DAG (1): 0: one launch per level and size class (round 1 / 2 schedule)
	int dag_split;            // SPP_DAG_SPLIT (1): the bottom of a large tree as a launch of its own; 0: one launch, 2: split whatever the size
	long long dag_timeout_ticks; // SPP_DAG_TIMEOUT_TICKS (5e7 = 0.5 s): bound of a flag wait inside the dependency-driven launch (debugging / tests: a tiny value forces the timeout fallback)
	int dag_trace;            // SPP_DAG_TRACE (off): n: the n-th factorization prints per-level start / children-done / end times
};

inline int env_int(const char *name, int dflt)
{
	const char *e = getenv(name);
	return e ? atoi(e) : dflt;
}

inline long long env_i64(const char *name, long long dflt)
{
	const char *e = getenv(name);
	return e ? atoll(e) : dflt;
}

inline double env_double(const char *name, double dflt)
{
	const char *e = getenv(name);
	return e ? atof(e) : dflt;
}

inline Switches parse_switches()
{
	Switches w;
	w.verbose = getenv("SPP_VERBOSE") != nullptr;
	const char *threads = getenv("SPP_PLAN_THREADS");
	w.plan_threads = threads ? std::max(1, atoi(threads)) : 0;
	w.plan_min_work = std::max<int64_t>(1, env_i64("SPP_PLAN_MIN_WORK", int64_t(1) << 18));

	w.dense_sched = env_int("SPP_DENSE_SCHED", 1);
	w.fused = env_int("SPP_FUSED", 1);
	w.aux_reserve_cus = env_int("SPP_AUX_RESERVE_CUS", 32);
	w.tile_444 = env_int("SPP_TILE_444", 0);
	w.dense_la = env_int("SPP_DENSE_LA", 0);
	w.la_chain_mask = env_int("SPP_LA_CHAIN_MASK", 1);
	w.la_g2 = env_int("SPP_LA_G2", 0);
	w.la_bulk_acquire = env_int("SPP_LA_BULK_ACQUIRE", 1);
	w.la_slots = env_i64("SPP_LA_SLOTS", 0);
	w.la_trace = env_int("SPP_LA_TRACE", 0);
	w.tail_rows = env_int("SPP_DENSE_TAIL", 1) ? env_int("SPP_TAIL_ROWS", 44) : 0;
	w.tail_mask = env_int("SPP_TAIL_MASK", 1);
	w.tail_order_beta = env_double("SPP_TAIL_ORDER_BETA", 0.0);
	w.tail_early = env_int("SPP_TAIL_EARLY", 1);
	w.tail_step_order = env_int("SPP_TAIL_STEP_ORDER", 1);
	w.tail_early_lead = env_int("SPP_TAIL_EARLY_LEAD", 1);
	w.tail_timeout_ticks = env_i64("SPP_TAIL_TIMEOUT_TICKS", WAIT_TICKS_DEFAULT);
	w.tail_trace = env_int("SPP_TAIL_TRACE", 0);
	w.trsv_chain = env_int("SPP_TRSV_CHAIN", 2);
	w.trsv_mform = env_int("SPP_TRSV_MFORM", 1);
	w.chain_timeout_ticks = env_i64("SPP_CHAIN_TIMEOUT_TICKS", WAIT_TICKS_DEFAULT);
	w.trsm_fused = env_int("SPP_TRSM_FUSED", 1);

	w.sacc_ulm = env_int("SPP_SACC_ULM", 1) != 0;
	w.sacc_factored = env_int("SPP_SACC_FACTORED", 1) != 0;
	w.sacc_tile = std::max<int64_t>(1, env_i64("SPP_SACC_TILE", 4));
	w.sacc_tile_cols = env_i64("SPP_SACC_TILE_COLS", -2);
	w.sacc_xcd = env_int("SPP_SACC_XCD", 1);
	w.sacc_chunk = env_int("SPP_SACC_CHUNK", 1);
	w.schur_cam_order = env_int("SPP_SCHUR_CAM_ORDER", 1);
	w.backsubst_fused = env_int("SPP_BACKSUBST_FUSED", 1);
	w.schur_side = env_int("SPP_SCHUR_SIDE", 1);
	w.solve_async = env_int("SPP_SOLVE_ASYNC", 1);
	w.lm_stream = env_int("SPP_LM_STREAM", 1);

	w.mid_front_max = std::max(128, std::min(MID_FRONT_MAX, env_int("SPP_MID_FRONT_MAX", 320)));
	const char *ordering = getenv("SPP_ORDERING");
	w.ordering = !ordering ? ORDERING_AUTO : (!strcmp(ordering, "nd") ? ORDERING_ND : ORDERING_AMD);
	w.amalg_small = env_i64("SPP_AMALG_SMALL", 32);
	w.amalg_zeros = env_double("SPP_AMALG_ZEROS", 0.12);
	w.amalg_relax_h = env_i64("SPP_AMALG_RELAX_H", 96);
	w.amalg_zeros_small = env_double("SPP_AMALG_ZEROS_SMALL", 0.2);
	w.sparse_teams = env_int("SPP_SPARSE_TEAMS", 1) != 0;
	w.sparse_team_max = std::max(1, std::min(64, env_int("SPP_SPARSE_TEAM_MAX", 40)));
	w.sparse_team_cols = std::max(8, std::min(256, env_int("SPP_SPARSE_TEAM_COLS", 16)));
	w.sparse_dag = env_int("SPP_SPARSE_DAG", 1);
	w.dag_split = env_int("SPP_DAG_SPLIT", 1);
	w.dag_timeout_ticks = env_i64("SPP_DAG_TIMEOUT_TICKS", WAIT_TICKS_DEFAULT);
	w.dag_trace = env_int("SPP_DAG_TRACE", 0);
	return w;
}

// parsed on the first call, by one thread (the initialization of a function-local static), and constant from then on
inline const Switches &switches()
{
	static const Switches w = parse_switches();
	return w;
}

} // namespace spp
