// spp_tile_plan.cpp -- host-side tile planning of the dense factor (integer work on 128 x 128 tile masks): which tiles
// of a reduced system are structurally nonzero (tile_mask_mark, tile_mask_close), which workgroup of the streamed launch
// takes which tile (tail_order_table), everything else the host decides for that launch (tail_plan), in which order a tile
// applies its steps (tail_step_order), and the cost model of that launch on a filled mask (tile_dag_cost).

#include "spp_internal.h"
#include <algorithm>

namespace spp {

// --------------------------------------------------------------------------------------------------
// Tile structure of a dense reduced system (the streamed dense factor, spp_dense_tail.h, skips structurally zero tiles).
// A word per tile row of DENSE_NB rows, bit j = tile (i, j); the layout is the factor's: n pivots, the right-hand side
// in column n, identity padding behind it (diagonal tiles only).
// --------------------------------------------------------------------------------------------------
void tile_mask_mark(int64_t n, int bs, int64_t nblk, const int32_t *i1, const int32_t *i2, std::vector<uint64_t> &words)
{
	words.clear();
	const int64_t Tr = (n + DENSE_NB - 1) / DENSE_NB, Tc = n / DENSE_NB + 1;
	if(Tr < 1 || Tc > 64)
		return; // (empty: every tile)
	words.assign((size_t)Tr, 0);
	for(int64_t q = 0; q < nblk; ++ q) {
		const int64_t a = std::min(i1[q], i2[q]), b = std::max(i1[q], i2[q]);
		// a bs x bs block may straddle two tiles in either direction
		const int64_t r0 = a * bs / DENSE_NB, r1 = std::min<int64_t>(a * bs + bs - 1, n - 1) / DENSE_NB;
		const int64_t c0 = b * bs / DENSE_NB, c1 = std::min<int64_t>(b * bs + bs - 1, n - 1) / DENSE_NB;
		if(a < 0 || r0 >= Tr || c0 >= Tr)
			continue;
		words[r0] |= (1ull << c0) | (1ull << c1);
		words[r1] |= (1ull << c0) | (1ull << c1);
	}
}

int64_t tile_mask_close(int64_t n, bool has_rhs, bool fill, std::vector<uint64_t> &words)
{
	const int64_t Tr = (n + DENSE_NB - 1) / DENSE_NB, Tc = has_rhs ? n / DENSE_NB + 1 : Tr;
	if(Tr < 1 || Tc > 64 || (int64_t)words.size() != Tr) {
		words.clear();
		return -1;
	}
	const uint64_t cols = Tc == 64 ? ~0ull : (1ull << Tc) - 1;
	for(int64_t i = 0; i < Tr; ++ i) {
		words[i] |= 1ull << i;
		if(has_rhs)
			words[i] |= 1ull << (n / DENSE_NB); // the tile column of the right-hand side is nonzero in every row
		words[i] &= cols & ~((1ull << i) - 1);
	}
	int64_t updates = 0;
	for(int64_t k = 0; k < Tr; ++ k) {
		const uint64_t r = words[k] & ~((2ull << k) - 1); // nonzero tiles right of the diagonal
		for(uint64_t m = r; m; m &= m - 1) {
			const int a = __builtin_ctzll(m);
			if(a >= Tr)
				break;
			const uint64_t f = r & ~((1ull << a) - 1);
			if(fill)
				words[a] |= f;
			updates += __builtin_popcountll(words[a] & f);
		}
	}
	return updates;
}

// Workgroup -> tile of the streamed launch (spp_dense_tail.h). bits[k + 1], bit j: tile (k, j) of the region is listed,
// bits[0]: the row panel in front of the region (step -1, applied only with have_pre).
// Tile (i, j) needs row tiles of (k, i) and (k, j), k < i, so any key alpha i + beta j with alpha > 0, beta >= 0 sorts the
// tiles topologically: that is the base order (beta = 0: row by row), and with !early the whole table.
// early: a set E of tiles goes in front of it, those that the base order seats many steps after their first update is
// out and that then run behind the chain until it has to wait for them.
//   first(i, j) = the first step tile (i, j) applies (bits i and j of that step's word both set), its own row i if none;
//   D = resident / (tiles of the widest listed row): whole rows the launch holds resident at its start;
//   a tile lags if i - first(i, j) > D;
//   E = the tiles of the longest run of trailing rows r* .. Tr - 1 in which every listed tile lags.
// Consumers of a tile of row i lie in rows > i, so a trailing run of rows is closed under "consumer of": NO TILE OUTSIDE E
// WAITS FOR A TILE OF E. The tiles outside E keep the base order among themselves -- topological --, so with E seated
// they complete one after the other on whatever is left, and then E does (row by row inside E). Progress needs
// resident > |E| instead of nothing at all; E is used only if
//   |E| <= resident / 2   and   resident - |E| >= max over r of #{(i, j) outside E : first(i, j) <= r <= i}
// (the live demand: tiles that have something to do while the chain is at row r), otherwise the table is the base
// order, entry for entry. info (may be null): {|E|, r*, D, live demand, widest row} -- r* = Tr, |E| = 0 when E is not used.
// lead (the caller sets it only together with a step order other than k ascending, tail_step_order below): a run that
// fails these conditions -- the 20 separator rows of a dissected Venice order, 210 tiles against 128 -- is not given up.
// E becomes its LEADING rows r* .. r2, the largest r2 with
//   |E| <= resident / 2   and   resident - |E| >= the live demand of the tiles of rows < r*   (as above),
// and the table is E, then the rows < r*, then the rows > r2. The rows < r* are numbered by the depth of their diagonal
// tile (ties: the base order) and not row by row: they are the chains that run side by side, each of which needs its
// next rows resident, and row by row the workgroups E leaves them all go to the first chain (measured, DESIGN section
// 25). Progress:
//   a tile of a row < r* waits for tiles of rows above its own alone -- never for E, never for a row > r2 --, a listed tile
//   (k, i), k < i, makes depth(k) < depth(i), so depth then base order is topological among them: with E seated they
//   complete one after the other on the resident - |E| >= 1 workgroups that are left;
//   a tile of E waits for tiles of rows < r* and for tiles of E in rows above its own, numbered before it inside E: E
//   completes row by row once the rows < r* have;
//   a tile of a row > r2 waits for smaller indices only.
// (Unlike the whole run the leading rows are not closed under "consumer of": the rows > r2 consume E, from behind it in
// the numbering.) The step order is what makes the seats pay: a tile of E, resident from the start, takes the steps of
// all chains as they come out and is level with them when the longest one ends; k ascending it would sit on its
// workgroup through the whole first chain with the others' row tiles piling up. With lead off the table is as before.
void tail_order_table(const std::vector<uint64_t> &bits, int Tr, int Tc, bool have_pre, double beta, int resident, bool early,
	std::vector<int> &order, int *info, bool lead)
{
	std::vector<std::pair<double, int> > key;
	for(int i = 0; i < Tr; ++ i)
		for(int j = i; j < Tc; ++ j)
			if((bits[(size_t)i + 1] >> j) & 1) // (only nonzero tiles get a workgroup)
				key.push_back(std::make_pair((double)i + beta * (double)j, (i << 16) | j));
	std::stable_sort(key.begin(), key.end(), [](const std::pair<double, int> &x, const std::pair<double, int> &y) { return x.first < y.first; });
	order.resize(key.size());
	for(size_t q = 0; q < key.size(); ++ q)
		order[q] = key[q].second;
	int widest = 1;
	for(int i = 0; i < Tr; ++ i)
		widest = std::max(widest, (int)__builtin_popcountll(bits[(size_t)i + 1]));
	const int D = std::max(resident, 0) / widest;
	if(info) {
		info[0] = 0;
		info[1] = Tr;
		info[2] = D;
		info[3] = 0;
		info[4] = widest;
	}
	if(!early || resident <= 0)
		return;
	auto first_step = [&](const int i, const int j) -> int {
		for(int k = have_pre ? -1 : 0; k < i; ++ k) {
			const uint64_t w = bits[(size_t)k + 1];
			if((w >> i) & (w >> j) & 1)
				return k;
		}
		return i;
	};
	int r_star = Tr;
	for(int i = Tr - 1; i >= 0; -- i) {
		bool all_lag = true;
		for(int j = i; j < Tc && all_lag; ++ j)
			if((bits[(size_t)i + 1] >> j) & 1)
				all_lag = i - first_step(i, j) > D;
		if(!all_lag)
			break;
		r_star = i;
	}
	int n_early = 0;
	std::vector<int> live((size_t)Tr + 1, 0); // (as differences first: +1 at first(i, j), -1 behind row i)
	for(size_t q = 0; q < order.size(); ++ q) {
		const int i = order[q] >> 16, j = order[q] & 0xffff;
		if(i >= r_star)
			++ n_early;
		else {
			++ live[(size_t)std::max(first_step(i, j), 0)];
			-- live[(size_t)i + 1];
		}
	}
	int demand = 0;
	for(int r = 0, run = 0; r < Tr; ++ r) {
		run += live[(size_t)r];
		demand = std::max(demand, run);
	}
	if(info)
		info[3] = demand;
	if(n_early == 0)
		return;
	if(n_early > resident / 2 || resident - n_early < demand) {
		if(!lead)
			return;
		// the leading rows r* .. r2 of the run (see above)
		const int room = std::min(resident / 2, resident - demand);
		int r2 = r_star - 1, n_lead = 0;
		for(int i = r_star; i < Tr; ++ i) {
			const int row = (int)__builtin_popcountll(bits[(size_t)i + 1] & ~((1ull << i) - 1) & (Tc == 64 ? ~0ull : (1ull << Tc) - 1));
			if(n_lead + row > room)
				break;
			n_lead += row;
			r2 = i;
		}
		if(n_lead == 0)
			return;
		std::vector<int> depth((size_t)Tr, 1); // (of the diagonal tiles: tile_dag_cost's definition)
		for(int k = 0; k < Tr; ++ k)
			for(int j = 0; j < k; ++ j)
				if((bits[(size_t)j + 1] >> k) & 1)
					depth[k] = std::max(depth[k], depth[j] + 1);
		auto key = [&](const int t) { const int i = t >> 16; return i < r_star ? 1 + depth[i] : (i <= r2 ? 0 : 2 + Tr); };
		std::stable_sort(order.begin(), order.end(), [&key](const int x, const int y) { return key(x) < key(y); });
		if(info) {
			info[0] = n_lead;
			info[1] = r_star;
		}
		return;
	}
	std::stable_partition(order.begin(), order.end(), [r_star](const int t) { return (t >> 16) >= r_star; });
	if(info) {
		info[0] = n_early;
		info[1] = r_star;
	}
}

bool is_permutation(const int32_t *v, int64_t n)
{
	std::vector<char> seen((size_t)n, 0);
	for(int64_t q = 0; q < n; ++ q) {
		if(v[q] < 0 || v[q] >= n || seen[(size_t)v[q]])
			return false;
		seen[(size_t)v[q]] = 1;
	}
	return true;
}

// The streamed launch (spp_dense_tail.h) takes everything behind row panel k -- the update of step k, then steps k + 1 .. --
// when that trailing matrix is a full factorization (every tile row a pivot block) of at most tail_rows tile rows (0: the
// launch is switched off) and TAIL_MAX_ROWS tile columns, the right-hand side's included. More tiles than CUs are fine:
// workgroups are dispatched in table order and leave after their own step, a workgroup that starts late finds the row
// tiles of the steps it missed in memory and catches up at the speed of its matrix cores.
//   Step words: from the caller's filled mask of the whole matrix (global tile indices; a sub-pattern of a filled pattern
// that starts at a later step is filled too) with tail_mask, else every tile; the diagonal tile always, nothing below it.
//   Step list: the row panel in front of the region first, then k ascending, or the caller's step order where the launch is
// the whole factorization -- with or without its mask in force (tail_mask changes scheduling, never bits).
//   Table: tail_order_table above. Lagging trailing rows go first (early) only with a mask in force; the leading rows of a
// run too large to be seated whole (lead) only under a step order other than k ascending, where a seated tile keeps level
// with the chains that feed it.
TailPlan tail_plan(const std::vector<uint64_t> *mask, const std::vector<int32_t> *step_order, int64_t nsteps, int64_t rows,
	int64_t ncols, int64_t k, int resident, const TailSwitches &sw, TailPlan *former)
{
	TailPlan p;
	const int64_t f = k + 1; // tile rows eliminated in front of the region
	const int64_t Tr = nsteps - f, Tc = (ncols - f * DENSE_NB + DENSE_NB - 1) / DENSE_NB;
	if(nsteps * DENSE_NB < rows || Tr < 1 || Tr > sw.tail_rows || Tc < Tr || Tc > Tr + 1 || Tc > TAIL_MAX_ROWS)
		return p;
	p.applies = true;
	TailPlan::Key &key = p.key;
	key.Tr = (int)Tr;
	key.Tc = (int)Tc;
	key.have_pre = f > 0;
	if(!sw.tail_mask || (mask && (int64_t)mask->size() != nsteps))
		mask = nullptr;
	p.masked = mask != nullptr;
	const uint64_t all_cols = Tc == 64 ? ~0ull : (1ull << Tc) - 1;
	key.rowbits.resize((size_t)Tr + 1);
	for(int64_t i = -1; i < Tr; ++ i) {
		uint64_t w = (mask && f + i >= 0) ? ((*mask)[(size_t)(f + i)] >> f) : all_cols;
		if(i >= 0)
			w = (w | (1ull << i)) & ~((1ull << i) - 1);
		key.rowbits[(size_t)i + 1] = w & all_cols;
	}
	p.ordered = f == 0 && step_order && (int64_t)step_order->size() == nsteps;
	bool ascending = true;
	int list[TAIL_MAX_ROWS + 1], n = 0;
	if(p.ordered) // (the kernel indexes its step words with these)
		SPP_REQUIRE(is_permutation(step_order->data(), Tr), SPP_E_BADARG, "streamed tail: the step order is not a permutation of the tile rows");
	if(key.have_pre)
		list[n ++] = -1;
	for(int q = 0; q < (int)Tr; ++ q) {
		list[n ++] = p.ordered ? (*step_order)[(size_t)q] : q;
		ascending = ascending && list[n - 1] == q;
	}
	tail_sorder_pack(p.sorder, list, n);
	key.early = p.masked && sw.tail_early != 0;
	key.lead = key.early && !ascending && sw.tail_early_lead != 0;
	p.resident = key.early ? resident : 0;
	if(former && former->key == key) {
		p.table.swap(former->table);
		std::copy(former->info, former->info + 5, p.info);
		return p;
	}
	p.table_fresh = true;
	tail_order_table(key.rowbits, key.Tr, key.Tc, key.have_pre, sw.tail_order_beta, p.resident, key.early, p.table, p.info, key.lead);
	return p;
}

// The order in which a tile of the streamed launch applies its steps (spp_dense_tail.h): the steps sorted by the depth of
// their diagonal tile in the tile DAG -- depth(k) = 1 + max depth(j) over j < k with tile (j, k) listed, 1 without such a
// j: the definition of tile_dag_cost below --, ties by k. Two chains that do not see each other (the arcs of a dissected
// camera order) emit their row tiles side by side, step m of either at about m chain steps into the launch, and that
// is the order of their depths: a tile that both update takes the steps as they come out instead of waiting for the whole
// first chain with the second one's row tiles long in memory. Along every dependency path the depth grows, so a chain
// (a band, a bordered band) keeps k ascending: the identity. A function of the filled mask alone.
void tail_step_order(const std::vector<uint64_t> &filled, std::vector<int32_t> &order)
{
	const int Tr = (int)std::min<size_t>(filled.size(), 64);
	std::vector<int> depth((size_t)Tr, 1);
	for(int k = 0; k < Tr; ++ k)
		for(int j = 0; j < k; ++ j)
			if((filled[(size_t)j] >> k) & 1)
				depth[k] = std::max(depth[k], depth[j] + 1);
	order.resize((size_t)Tr);
	for(int k = 0; k < Tr; ++ k)
		order[k] = k;
	std::stable_sort(order.begin(), order.end(), [&depth](const int32_t x, const int32_t y) { return depth[x] < depth[y]; });
}

TileDagCost tile_dag_cost(int64_t n, const std::vector<uint64_t> &filled, int resident)
{
	TileDagCost c;
	const int64_t Tr = (int64_t)filled.size();
	std::vector<uint64_t> w(filled);
	c.updates = tile_mask_close(n, true, true, w); // (closed already: counts the updates)
	std::vector<int> depth((size_t)Tr, 1);
	for(int64_t k = 0; k < Tr; ++ k) {
		c.tiles += __builtin_popcountll(w[k]);
		for(int64_t j = 0; j < k; ++ j)
			if((w[j] >> k) & 1)
				depth[k] = std::max(depth[k], depth[j] + 1);
		c.path = std::max<int64_t>(c.path, depth[k]);
	}
	c.cost_us = std::max(c.path * TAIL_MODEL_STEP_US, c.updates * TAIL_MODEL_UPDATE_US / std::max(1, resident)) + TAIL_MODEL_START_US;
	return c;
}

} // namespace spp
