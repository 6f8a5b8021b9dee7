// How rb2_hip_string_graph (kernels: rb2_graph.h; host side: rb2_query_host.h) cuts the sources into chunks of whole
// strings: the arithmetic alone, plain C++ with no HIP in it, so that a CPU program can include it (tests/test_graph_plan.py).
//
// A chunk holds at most `limit` strings -- RB2_GRAPH_CHUNK, and what GRAPH_REC_BYTES of records hold at max_recs * 32 bytes a string --
// and at most GRAPH_TEXT_BYTES of packed text (every string with its closing 0); a single string is a chunk whatever it takes.  The
// lengths are known on the device only, so the host TRIES a number of strings: the device measures them, cuts them at the text budget
// (graph_text_cut, which is compiled for both sides) and tells the host how many the chunk TOOK, behind the one synchronise of the chunk.
// What a try measured and did not take is measured again by the next one, so after a cut the host tries a quarter more than was taken.
#pragma once
#include "rb2_query_plan.h"

static const int64_t GRAPH_TEXT_BYTES = (int64_t)256 << 20;    /* packed text of a chunk at the most (one string may be longer alone) */
static const int64_t GRAPH_REC_BYTES = (int64_t)256 << 20;     /* records of a chunk at the most: strings * max_recs * 32 (one string's may be more alone) */

/* strings of a chunk at the most: chunk (>= 1) of them, what GRAPH_REC_BYTES hold at max_recs (>= 1) records each, one at the least */
inline int64_t graph_chunk_limit(int64_t chunk, int64_t max_recs)
{
	return std::max<int64_t>(1, std::min(chunk, GRAPH_REC_BYTES / 32 / max_recs));
}

/* off[0 .. n]: the offsets of n (>= 1) strings tried, off[i + 1] - off[i] = the bytes of string i.  The strings the chunk takes: the
 * largest e in 1 .. n with off[e] - off[0] <= budget, and 1 when the first string alone is larger */
RB2_PLAN_HD inline int64_t graph_text_cut(const uint64_t *off, int64_t n, uint64_t budget)
{
	int64_t lo = 1, hi = n;
	while (lo < hi) {
		const int64_t mid = lo + (hi - lo + 1) / 2;
		if (off[mid] - off[0] <= budget) lo = mid; else hi = mid - 1;
	}
	return lo;
}

struct GraphPlan { int64_t limit, next; };             /* next: the strings the next chunk tries, 1 .. limit */

inline GraphPlan graph_plan(int64_t chunk, int64_t max_recs)
{
	const int64_t l = graph_chunk_limit(chunk, max_recs);
	return {l, l};
}

/* the strings to try when `left` (>= 1) are left */
inline int64_t graph_try(const GraphPlan &p, int64_t left) { return std::min(p.next, left); }

/* the chunk took `took` (1 .. tried) of the strings tried: cut by the text, the next one tries a quarter more than fitted; whole, twice as many */
inline void graph_took(GraphPlan &p, int64_t tried, int64_t took)
{
	const int64_t want = took < tried ? took + took / 4 + 1 : 2 * tried;
	p.next = std::max<int64_t>(1, std::min(p.limit, want));
}
