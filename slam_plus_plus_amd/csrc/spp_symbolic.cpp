// spp_symbolic.cpp -- fill-reducing orderings of the block graph (host side, integer work, once per block structure).
//
//  * min_degree_order: the role of CMatrixOrdering::p_BlockOrdering, src/slam/OrderingMagic.cpp:701-1034, which calls
//    amd_l2. This is our own quotient-graph approximate-minimum-degree implementation written from the published
//    algorithm (Amestoy, Davis, Duff 1996); it is NOT the reference's AMD code and gives a different (equally valid)
//    elimination order. Delta-x parity does not depend on the order.
//  * nested_dissection_order: dissection on BFS level structures with minimum-degree leaves.

#include "spp_internal.h"
#include <algorithm>
#include <numeric>

namespace spp {

// --------------------------------------------------------------------------------------------------
// Approximate minimum degree on the block graph (A + A^T pattern of the upper-triangular input).
// Quotient graph with element absorption, approximate external degrees (|Le \ Lp| bound),
// mass elimination of indistinguishable variables is omitted (block graphs here are small).
// order[k] = block column eliminated k-th.
// --------------------------------------------------------------------------------------------------
void min_degree_order(int64_t nb, const int64_t *col_ptr, const int64_t *row_idx, std::vector<int64_t> &order)
{
	order.clear();
	order.reserve(nb);
	if(nb == 0)
		return;
	// adjacency (variables) of A + A^T without the diagonal
	std::vector<std::vector<int32_t> > adj(nb), elems(nb); // variable -> variable nbrs / element nbrs
	for(int64_t j = 0; j < nb; ++ j)
		for(int64_t p = col_ptr[j]; p < col_ptr[j + 1]; ++ p) {
			int64_t i = row_idx[p];
			if(i != j) {
				adj[i].push_back((int32_t)j);
				adj[j].push_back((int32_t)i);
			}
		}
	for(int64_t i = 0; i < nb; ++ i) {
		std::sort(adj[i].begin(), adj[i].end());
		adj[i].erase(std::unique(adj[i].begin(), adj[i].end()), adj[i].end());
	}
	std::vector<std::vector<int32_t> > elem_vars(nb); // element (named by its pivot) -> variables
	std::vector<uint8_t> state(nb, 0);               // 0 variable, 1 element, 2 absorbed element
	std::vector<int64_t> degree(nb);
	std::vector<int64_t> w(nb, -1);                  // |Le \ Lp| workspace, stamped
	std::vector<int64_t> mark(nb, -1);
	// degree buckets (doubly linked lists)
	std::vector<int32_t> head(nb + 1, -1), next(nb, -1), prev(nb, -1);
	auto bucket_insert = [&](int32_t v) {
		int64_t d = std::min<int64_t>(degree[v], nb);
		next[v] = head[d];
		prev[v] = -1;
		if(head[d] >= 0) prev[head[d]] = v;
		head[d] = v;
	};
	auto bucket_remove = [&](int32_t v) {
		int64_t d = std::min<int64_t>(degree[v], nb);
		if(prev[v] >= 0) next[prev[v]] = next[v]; else head[d] = next[v];
		if(next[v] >= 0) prev[next[v]] = prev[v];
	};
	for(int64_t i = 0; i < nb; ++ i) {
		degree[i] = (int64_t)adj[i].size();
		bucket_insert((int32_t)i);
	}
	int64_t mindeg = 0;
	std::vector<int32_t> Lp;
	for(int64_t step = 0; step < nb; ++ step) {
		while(mindeg <= nb && head[mindeg] < 0)
			++ mindeg;
		const int32_t p = head[mindeg];
		bucket_remove(p);
		order.push_back(p);
		// Lp = adj(p) U (union of Le for e in elems(p)) \ {p}
		Lp.clear();
		mark[p] = step;
		for(size_t q = 0; q < adj[p].size(); ++ q) {
			int32_t v = adj[p][q];
			if(state[v] == 0 && mark[v] != step) {
				mark[v] = step;
				Lp.push_back(v);
			}
		}
		for(size_t q = 0; q < elems[p].size(); ++ q) {
			int32_t e = elems[p][q];
			if(state[e] != 1)
				continue;
			for(size_t t = 0; t < elem_vars[e].size(); ++ t) {
				int32_t v = elem_vars[e][t];
				if(state[v] == 0 && mark[v] != step) {
					mark[v] = step;
					Lp.push_back(v);
				}
			}
			state[e] = 2; // absorbed into p
			std::vector<int32_t>().swap(elem_vars[e]);
		}
		state[p] = 1;
		std::vector<int32_t>().swap(adj[p]);
		std::vector<int32_t>().swap(elems[p]);
		elem_vars[p] = Lp;
		const int64_t lp = (int64_t)Lp.size();
		// w(e) = |Le \ Lp| for every element adjacent to a variable of Lp
		for(size_t q = 0; q < Lp.size(); ++ q) {
			int32_t v = Lp[q];
			for(size_t t = 0; t < elems[v].size(); ++ t) {
				int32_t e = elems[v][t];
				if(state[e] != 1)
					continue;
				if(w[e] < step * (nb + 1)) { // first touch in this step: stamp + live size
					int64_t sz = 0;
					for(size_t u = 0; u < elem_vars[e].size(); ++ u)
						if(state[elem_vars[e][u]] == 0)
							++ sz;
					w[e] = step * (nb + 1) + sz;
				}
				-- w[e];
			}
		}
		for(size_t q = 0; q < Lp.size(); ++ q) {
			const int32_t v = Lp[q];
			bucket_remove(v);
			// prune: variable neighbours inside Lp (now covered by element p) and dead entries
			{
				std::vector<int32_t> &a = adj[v];
				size_t o = 0;
				for(size_t t = 0; t < a.size(); ++ t)
					if(state[a[t]] == 0 && mark[a[t]] != step)
						a[o ++] = a[t];
				a.resize(o);
			}
			int64_t d = (int64_t)adj[v].size() + (lp - 1);
			{
				std::vector<int32_t> &el = elems[v];
				size_t o = 0;
				for(size_t t = 0; t < el.size(); ++ t) {
					int32_t e = el[t];
					if(state[e] != 1)
						continue;
					int64_t we = w[e] - step * (nb + 1);
					if(we <= 0) {
						// Le is a subset of Lp: aggressive absorption
						continue;
					}
					d += we;
					el[o ++] = e;
				}
				el.resize(o);
				el.push_back(p);
			}
			degree[v] = std::min<int64_t>(std::min<int64_t>(d, nb - step - 1), degree[v] + lp - 1);
			if(degree[v] < 0) degree[v] = 0;
			bucket_insert(v);
			if(degree[v] < mindeg)
				mindeg = degree[v];
		}
	}
}


// --------------------------------------------------------------------------------------------------
// Nested dissection on the block graph (George & Liu's automatic nested dissection): a level
// structure rooted at a pseudo-peripheral vertex, the smallest level of its middle part as vertex
// separator (thinned to the vertices that really touch the far side), recursion on the two parts,
// separator ordered last; subdomains of at most ND_LEAF blocks are ordered by minimum degree.
// Chain-like graphs (the reduced camera system of a long trajectory, BASELINE config 5) get an
// elimination tree of logarithmic height instead of the one long chain minimum degree produces, which
// is what the level-scheduled multifrontal kernels need (ordering).
// order[k] = block column eliminated k-th.
// --------------------------------------------------------------------------------------------------
static const int ND_LEAF = 48;

void nested_dissection_order(int64_t nb, const int64_t *col_ptr, const int64_t *row_idx, std::vector<int64_t> &order)
{
	order.assign(nb, -1);
	if(nb == 0)
		return;
	std::vector<std::vector<int32_t> > adj(nb);
	for(int64_t j = 0; j < nb; ++ j)
		for(int64_t p = col_ptr[j]; p < col_ptr[j + 1]; ++ p) {
			const int64_t i = row_idx[p];
			if(i != j) {
				adj[i].push_back((int32_t)j);
				adj[j].push_back((int32_t)i);
			}
		}
	// part[v]: id of the subset v currently belongs to; subsets are processed from a stack, each gets
	// a target range [lo, hi) of positions in the final order (separator at the end of the range)
	std::vector<int32_t> part(nb, 0), level(nb, -1), local(nb, -1);
	struct Task { std::vector<int32_t> verts; int64_t lo; };
	std::vector<Task> stack;
	{
		Task t;
		t.verts.resize(nb);
		for(int64_t v = 0; v < nb; ++ v)
			t.verts[v] = (int32_t)v;
		t.lo = 0;
		stack.push_back(std::move(t));
	}
	int32_t next_part = 1;
	std::vector<int32_t> queue;
	auto bfs = [&](int32_t root, int32_t pid, std::vector<int32_t> &out) { // level structure inside subset pid
		out.clear();
		out.push_back(root);
		level[root] = 0;
		for(size_t h = 0; h < out.size(); ++ h) {
			const int32_t v = out[h];
			for(size_t q = 0; q < adj[v].size(); ++ q) {
				const int32_t u = adj[v][q];
				if(part[u] == pid && level[u] < 0) {
					level[u] = level[v] + 1;
					out.push_back(u);
				}
			}
		}
	};
	while(!stack.empty()) {
		Task t = std::move(stack.back());
		stack.pop_back();
		const int64_t m = (int64_t)t.verts.size();
		if(m == 0)
			continue;
		const int32_t pid = part[t.verts[0]];
		if(m <= ND_LEAF) {
			// minimum degree on the induced subgraph (upper pattern in local numbering)
			for(int64_t q = 0; q < m; ++ q)
				local[t.verts[q]] = (int32_t)q;
			std::vector<int64_t> cp(m + 1, 0), ri;
			for(int64_t q = 0; q < m; ++ q) {
				const int32_t v = t.verts[q];
				for(size_t e = 0; e < adj[v].size(); ++ e) {
					const int32_t u = adj[v][e];
					if(part[u] == pid && local[u] < q)
						ri.push_back(local[u]);
				}
				std::sort(ri.begin() + cp[q], ri.end());
				ri.erase(std::unique(ri.begin() + cp[q], ri.end()), ri.end());
				ri.push_back(q); // diagonal last
				cp[q + 1] = (int64_t)ri.size();
			}
			std::vector<int64_t> lo;
			min_degree_order(m, cp.data(), ri.data(), lo);
			for(int64_t q = 0; q < m; ++ q)
				order[t.lo + q] = t.verts[lo[q]];
			for(int64_t q = 0; q < m; ++ q) {
				local[t.verts[q]] = -1;
				part[t.verts[q]] = -1; // done
			}
			continue;
		}
		// pseudo-peripheral root: two sweeps
		bfs(t.verts[0], pid, queue);
		if((int64_t)queue.size() < m) {
			// disconnected: split off this component, no separator
			const int32_t pa = next_part ++;
			Task a, b;
			for(size_t q = 0; q < queue.size(); ++ q)
				part[queue[q]] = pa;
			for(int64_t q = 0; q < m; ++ q) {
				const int32_t v = t.verts[q];
				level[v] = -1;
				(part[v] == pa ? a : b).verts.push_back(v);
			}
			a.lo = t.lo;
			b.lo = t.lo + (int64_t)a.verts.size();
			stack.push_back(std::move(a));
			stack.push_back(std::move(b));
			continue;
		}
		int32_t far = queue.back();
		for(size_t q = 0; q < queue.size(); ++ q)
			level[queue[q]] = -1;
		bfs(far, pid, queue);
		const int32_t nlev = level[queue.back()] + 1;
		if(nlev < 3) { // clique-like: no useful separator
			for(int64_t q = 0; q < m; ++ q) {
				local[t.verts[q]] = (int32_t)q;
				level[t.verts[q]] = -1;
			}
			std::vector<int64_t> cp(m + 1, 0), ri;
			for(int64_t q = 0; q < m; ++ q) {
				const int32_t v = t.verts[q];
				for(size_t e = 0; e < adj[v].size(); ++ e) {
					const int32_t u = adj[v][e];
					if(part[u] == pid && local[u] < q)
						ri.push_back(local[u]);
				}
				std::sort(ri.begin() + cp[q], ri.end());
				ri.erase(std::unique(ri.begin() + cp[q], ri.end()), ri.end());
				ri.push_back(q);
				cp[q + 1] = (int64_t)ri.size();
			}
			std::vector<int64_t> lo;
			min_degree_order(m, cp.data(), ri.data(), lo);
			for(int64_t q = 0; q < m; ++ q)
				order[t.lo + q] = t.verts[lo[q]];
			for(int64_t q = 0; q < m; ++ q) {
				local[t.verts[q]] = -1;
				part[t.verts[q]] = -1;
			}
			continue;
		}
		// level sizes; separator = smallest level whose cumulative position lies in the middle part
		std::vector<int64_t> lsize(nlev, 0);
		for(size_t q = 0; q < queue.size(); ++ q)
			++ lsize[level[queue[q]]];
		int32_t best = -1;
		{
			int64_t below = 0;
			double best_cost = 0;
			for(int32_t l = 0; l < nlev; ++ l) {
				const int64_t above = m - below - lsize[l];
				if(l > 0 && l + 1 < nlev) {
					const double bal = (double)std::min(below, above) / (double)std::max<int64_t>(1, std::max(below, above));
					// small separators, balanced parts: separator size penalized by imbalance
					const double cost = (double)lsize[l] * (1.0 + 2.0 * (1.0 - bal) * (1.0 - bal) * 4.0);
					if(bal >= 0.25 && (best < 0 || cost < best_cost)) {
						best = l;
						best_cost = cost;
					}
				}
				below += lsize[l];
			}
			if(best < 0)
				best = nlev / 2;
		}
		// near part: levels < best; far part: levels > best; separator vertices without a neighbour in
		// level best + 1 move to the near part
		const int32_t pa = next_part ++, pb = next_part ++;
		Task a, b;
		std::vector<int32_t> sep;
		for(size_t q = 0; q < queue.size(); ++ q) {
			const int32_t v = queue[q];
			if(level[v] < best)
				a.verts.push_back(v);
			else if(level[v] > best)
				b.verts.push_back(v);
			else {
				bool touches = false;
				for(size_t e = 0; e < adj[v].size() && !touches; ++ e) {
					const int32_t u = adj[v][e];
					touches = part[u] == pid && level[u] == best + 1;
				}
				if(touches)
					sep.push_back(v);
				else
					a.verts.push_back(v);
			}
		}
		for(size_t q = 0; q < a.verts.size(); ++ q)
			part[a.verts[q]] = pa;
		for(size_t q = 0; q < b.verts.size(); ++ q)
			part[b.verts[q]] = pb;
		for(size_t q = 0; q < queue.size(); ++ q)
			level[queue[q]] = -1;
		a.lo = t.lo;
		b.lo = t.lo + (int64_t)a.verts.size();
		const int64_t slo = b.lo + (int64_t)b.verts.size();
		for(size_t q = 0; q < sep.size(); ++ q) {
			order[slo + (int64_t)q] = sep[q];
			part[sep[q]] = -1;
		}
		stack.push_back(std::move(a));
		stack.push_back(std::move(b));
	}
}

} // namespace spp

