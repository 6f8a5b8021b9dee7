// The arithmetic of the approximate search with insertions and deletions (rb2_hip_approx_ed: kernel k_approx_ed in rb2_edit.h, host side in
// rb2_query_host.h): the packed column of the dynamic programme and the stack of a row.  The rows and the launches
// of a call follow from that stack by stack_rows, stack_len_cap and stack_passes of rb2_query_plan.h, as for rb2_hip_approx.
// Plain C++ with no HIP in it: the kernel and a CPU program (tests/edit_plan_check.cpp) compile the same text.
#pragma once
#include "rb2_query_plan.h"

/* The words.  q = the query, L symbols; z = the last symbol of a match S, a = its first one, W' = what lies between them, built from its
 * last symbol as a backward search meets it; t = q[1 .. L - 1) is the inner target, M = L - 2 symbols.  The node of the word W'z at depth
 * d = |W'| carries the column D[j] = lev(W', t[j:]), j = 0 .. M, and c0 = sub(z, q[L - 1]).
 * The band.  D[j] >= |d - (M - j)|, so only the cells with |j - (M - d)| <= max_ed can hold a value of max_ed or less.  max_ed <= 4: a
 * column is EDIT_CELLS = 9 fields of 4 bits in one word, field b = the cell j = M - d + b - 4, every value capped at cap = max_ed + 1 and
 * a field whose j lies outside 0 .. M holding cap.  A capped value is never below min(the true one, cap): the band drops alignments, all of
 * which cost more than max_ed, and adds none. */
static const int EDIT_MAX_ED = 4;                              /* edits of a match at the most: the band is 2 * 4 + 1 cells */
static const int EDIT_CELLS = 2 * EDIT_MAX_ED + 1;
static const int EDIT_NONE = 15;                               /* in a window: the field has no cell (j outside 0 .. M) */

constexpr int edit_sub(int a, int c) { return !(a == c && c >= 1 && c <= 4); }            /* the cost of a column: an N equals nothing */
constexpr int edit_cell(uint64_t w, int b) { return (int)(w >> (4 * b) & 15); }
constexpr uint64_t edit_put(int b, int v) { return (uint64_t)v << (4 * b); }
constexpr int64_t edit_j(int64_t M, int64_t d, int b) { return M - d + b - EDIT_MAX_ED; } /* the cell of field b at depth d */

/* the column of the empty W' (depth 0): D[j] = M - j */
RB2_PLAN_HD inline uint64_t edit_init(int64_t M, int cap)
{
	uint64_t col = 0;
	for (int b = 0; b < EDIT_CELLS; ++b) {
		const int64_t j = edit_j(M, 0, b);
		col |= edit_put(b, j >= 0 && j <= M && M - j < cap ? (int)(M - j) : cap);
	}
	return col;
}

/* what the step to depth d (>= 0; the initial column is depth 0) reads of the query, one field per cell of the new column: t[j] = q[j + 1]
 * for j < M, 0 for j = M (a cell with no diagonal), EDIT_NONE for a field without a cell.  The same for the four children of a node. */
RB2_PLAN_HD inline uint64_t edit_window(const uint8_t *q, int64_t M, int64_t d)
{
	uint64_t w = 0;
	for (int b = 0; b < EDIT_CELLS; ++b) {
		const int64_t j = edit_j(M, d, b);
		w |= edit_put(b, j < 0 || j > M ? EDIT_NONE : j == M ? 0 : (int)q[j + 1]);
	}
	return w;
}

/* the piece bound per cell of a column at depth d: approx_need(G, pieces, j + 1), the edits every match needs in q[0 .. j], which the
 * cell j does not cover (it stands for q[j + 1 .. L - 2]); EDIT_NONE for a field without a cell.  G = NULL: no bound (all zeros). */
RB2_PLAN_HD inline uint64_t edit_needs(const uint8_t *G, int pieces, int64_t M, int64_t d)
{
	uint64_t w = 0;
	for (int b = 0; b < EDIT_CELLS; ++b) {
		const int64_t j = edit_j(M, d, b);
		w |= edit_put(b, j < 0 || j > M ? EDIT_NONE : G ? approx_need(G, pieces, j + 1) : 0);
	}
	return w;
}

/* the column of aW' from the column of W': ND[M] = D[M] + 1, ND[j] = min(D[j] + 1, ND[j + 1] + 1, D[j + 1] + sub(a, t[j])).  win = the
 * window of the new depth.  Field b of the new column is the cell of field b - 1 of the old one, so D[j] = old[b - 1], D[j + 1] = old[b] */
RB2_PLAN_HD inline uint64_t edit_step(uint64_t col, uint64_t win, int a, int cap)
{
	uint64_t out = 0;
	int right = cap;                                           /* ND[j + 1], the field above */
	for (int b = EDIT_CELLS - 1; b >= 0; --b) {
		const int s = edit_cell(win, b);
		int v = cap;
		if (s != EDIT_NONE) {
			if (b > 0 && edit_cell(col, b - 1) + 1 < v) v = edit_cell(col, b - 1) + 1;
			if (right + 1 < v) v = right + 1;
			if (s != 0 && edit_cell(col, b) + edit_sub(a, s) < v) v = edit_cell(col, b) + edit_sub(a, s);
		}
		out |= edit_put(b, v);
		right = v;
	}
	return out;
}

/* D[0] of a column at depth d: field d - M + 4, cap when the band no longer holds it */
RB2_PLAN_HD inline int edit_d0(uint64_t col, int64_t M, int64_t d, int cap)
{
	const int64_t b = d - M + EDIT_MAX_ED;
	return b >= 0 && b < EDIT_CELLS ? edit_cell(col, (int)b) : cap;
}

/* the terminal test: ed(aW'z, q) = c0 + D[0] + sub(a, q[0]), or more than max_ed (returned as it comes: compare with max_ed) */
RB2_PLAN_HD inline int edit_terminal(uint64_t col, int64_t M, int64_t d, int cap, int c0, int a, int q0) { return c0 + edit_d0(col, M, d, cap) + edit_sub(a, q0); }

/* the live test: some cell of the column can still make a match, c0 + D[j] + need[j] <= max_ed (needs = edit_needs of the column's depth) */
RB2_PLAN_HD inline bool edit_live(uint64_t col, uint64_t needs, int c0, int max_ed)
{
	bool live = false;
	for (int b = 0; b < EDIT_CELLS; ++b) {
		const int nd = edit_cell(needs, b);
		live = live || (nd != EDIT_NONE && c0 + edit_cell(col, b) + nd <= max_ed);
	}
	return live;
}

/* The stack of one row for queries of up to L (>= 1) symbols.  A path is the root and up to L - 1 + max_ed nodes below it (z, then W' of
 * 1 .. M + max_ed symbols: a longer one has no live cell), so edit_nodes positions; per position the intervals of the four children (64
 * bytes: one line, as in k_approx), the column (8 bytes) and one byte "child taken | next to try << 3"; then G of approx_bound, one byte
 * per symbol of the query.  The byte arrays are padded to 8 bytes. */
constexpr int64_t edit_nodes(int64_t L, int max_ed) { return L + max_ed; }
constexpr int64_t edit_row_bytes(int64_t L, int max_ed) { return 72 * edit_nodes(L, max_ed) + approx_pad(edit_nodes(L, max_ed)) + approx_pad(L); }
