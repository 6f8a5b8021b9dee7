// rb2_edit.h -- approximate search with insertions and deletions on the device index (include/rb2_hip.h: rb2_hip_approx_ed; DESIGN.md
// section 27).  The arithmetic -- the packed column, the stack of a row -- is rb2_edit_plan.h, which a CPU program tests.
#pragma once
#include "rb2_query.h"
#include "rb2_edit_plan.h"

namespace rb2 {

// A match of the query q (L symbols) is a word S over A C G T with ed(S, q) <= max_ed and at least min_occ occurrences, ed being the
// unit-cost edit distance with the first and the last symbols of S aligned to those of q (include/rb2_hip.h).  Depth-first search over the
// trie of words, built from the last symbol: the root's child z is the last symbol of S (c0 = sub(z, q[L - 1])); below it the node of W'z
// carries the column D[j] = lev(W', q[1 + j .. L - 1)) as nine 4-bit fields of one word (rb2_edit_plan.h).  One pair of ranks of a node's
// interval gives the intervals of its four children a, as in k_approx; a child with min_occ rows is a match when c0 + D[0] + sub(a, q[0])
// <= max_ed (no rank: its interval is known), and is followed with the column of aW' when some cell j has c0 + ND[j] + need(j + 1) <=
// max_ed, need being the piece bound of approx_bound over the whole query.  A trie node is a distinct word: every match is met once.
//
// One query per DPP row, control uniform within the row; a row takes the queries i = row, row + rows, ... with lmin < L <= lcap (the host
// sorts the lengths into launches: stack_passes).  The stack is the path, in the row's part of scr (edit_row_bytes(lrow, max_ed) bytes), one
// position for the root (0) and one for each node below it (p = the symbols of its word):
//   kid[8 p + 2 (a - 1) ..] = lo, hi of child a of the node at p                (lanes 0 .. 7 store one word each: one 64-byte line)
//   col[p] = its column          tk[p] = the child taken at p | the next one to try << 3          G[x] = approx_bound's count
// so that coming back to a node costs loads and no rank: tk and col, and the kid line in one go when a child is left to try (the window
// of the query and of G is read only when a child with min_occ rows asks for it).  kid is the kid line of rb2_query.h (kid_store,
// kid_line) with its two fences.  col, tk and G are written by every lane with the same value, each lane reads its own.
// Every pair of ranks, those of the bound included, is a step: at max_steps the query ends with cnt = -2 - (matches found so far).  Between
// two steps a row looks at four children and pops at most what it pushed, and a word below the root is never longer than L - 1 + max_ed
// (a longer one has no live cell; the push checks the position against the stack besides), so a launch ends after n * max_steps pairs of
// ranks whatever the index holds.
// rec[(i * max_recs + k) * 4 ..] = lo, hi, ed, len for k < max_recs, by lanes 0 .. 3; cnt[i] as in include/rb2_hip.h.
template <bool SPARSE> __global__ __launch_bounds__(256) void k_approx_ed(const QTab *Tg, PoolView pv, const uint8_t *qry, const int64_t *off, int64_t base, uint64_t n,
                                                                          int max_ed, int64_t min_occ, int64_t max_steps, int64_t max_recs, int64_t lmin, int64_t lcap,
                                                                          uint64_t rows, int64_t lrow, uint8_t *scr, int64_t *rec, int64_t *cnt)
{
	__shared__ QTab T;
	qtab_load(Tg, T);
	const QRow R = qrow();
	if (R.i >= rows) return;
	const int64_t N = (int64_t)T.row0[NR], P = edit_nodes(lrow, max_ed);
	const int cap = max_ed + 1;
	uint64_t *kid = (uint64_t*)(scr + R.i * (uint64_t)edit_row_bytes(lrow, max_ed)), *colv = kid + 8 * P;
	uint8_t *tk = (uint8_t*)(colv + P), *G = tk + approx_pad(P);
	for (uint64_t i = R.i; i < n; i += rows) {
		const int64_t L = off[i + 1] - off[i];
		if (L <= lmin || L > lcap) continue;                       // another launch takes it
		const QSlice S = qslice<false>(qry, off, base, i, L > min(lrow, APPROX_MAX_LEN));   // (longer than the stack: malformed, and not read)
		if (S.bad || L == 0) { if (R.g == 0) cnt[i] = S.bad ? -1 : 0; continue; }
		int64_t steps = 0, k = 0;
		const int pieces = approx_bound(S.q, L, N, min_occ, max_ed, max_steps, [&](int64_t lo, int64_t hi, int c, int64_t &nlo, int64_t &nhi) {
			QPair<SPARSE>(T, pv, (uint64_t)lo, (uint64_t)hi).child(T, c, nlo, nhi); }, G, &steps);
		if (pieces < 0 || pieces > max_ed) { if (R.g == 0) cnt[i] = pieces < 0 ? -2 : 0; continue; }
		const int64_t M = L - 2;
		const int q0 = S.q[0], qz = S.q[L - 1];
		int64_t p = 0;
		uint64_t lo = 0, hi = (uint64_t)N, col = 0;
		int c0 = 0;
		bool over = false;
		for (;;) {                                                 // the node at p ([lo, hi), col, c0): its children, then the next node in depth-first order
			if (steps >= max_steps) { over = true; break; }
			++steps;
			uint64_t klo[4], khi[4];
			kid_store(T, QPair<SPARSE>(T, pv, lo, hi), kid, p, R.g, klo, khi);
			bool down = false;
			int t = 1;
			for (;;) {                                             // the children of the node at p from t on; with none left, back to the node above
				uint64_t win = 0, needs = 0;                       // what the four children share: the window and the bound of depth p, D[0] of this node,
				int d0 = cap;                                      // read when the first child with min_occ rows asks for them
				bool have = false;
				while (t <= 4) {
					const int a = t++;
					uint64_t xlo = 0, xhi = 0;
#pragma unroll
					for (int b = 0; b < 4; ++b) if (a == b + 1) { xlo = klo[b]; xhi = khi[b]; }
					if ((int64_t)(xhi - xlo) < min_occ) continue;
					if (!have && L >= 2) {
						win = edit_window(S.q, M, p);
						needs = edit_needs(G, pieces, M, p);
						if (p > 0) d0 = edit_d0(col, M, p - 1, cap);
						have = true;
					}
					uint64_t nc;
					int nc0 = c0;
					if (p == 0) {                                      // z: the last symbol of the match
						nc0 = edit_sub(a, qz);
						if (L == 1) {
							if (nc0 <= max_ed) { qstore(rec, i, max_recs, k, R.g, xlo, xhi, nc0, 1); ++k; }
							continue;
						}
						nc = edit_init(M, cap);
					} else {
						const int e = c0 + d0 + edit_sub(a, q0);       // a as the first symbol of the match
						if (e <= max_ed) { qstore(rec, i, max_recs, k, R.g, xlo, xhi, e, p + 1); ++k; }
						nc = edit_step(col, win, a, cap);              // a as one more inner symbol
					}
					if (p + 1 >= P || !edit_live(nc, needs, nc0, max_ed)) continue;
					tk[p] = (uint8_t)(a | t << 3);
					c0 = nc0; col = nc; lo = xlo; hi = xhi;
					colv[++p] = col; down = true;
					break;
				}
				if (down || p == 0) break;
				const int b = tk[--p];
				t = b >> 3;
				col = colv[p];                                         // (of the root: never read)
				__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
				if (t <= 4) kid_line(kid, p, klo, khi);                // the line of the node's children, in one go
			}
			if (!down) break;                                      // back at the root with no child left: the search is complete
		}
		if (R.g == 0) cnt[i] = over ? -2 - k : k;
	}
}

}  // namespace rb2
