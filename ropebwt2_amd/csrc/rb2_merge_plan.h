// The batch-cutting arithmetic of rb2_hip_merge that needs no GPU.  Plain C++, so that a CPU program can include
// it (tests/test_merge_plan.py).
//
// The strings of the source stand behind each other in one batch text: string i is off[i] .. off[i + 1], its symbols and its closing 0,
// so off[i + 1] - off[i] >= 1, off[0] = 0 and off[n] = total.  The offsets stay on the device; the host holds the block sums of the
// scan that made them, bsum[b] = off[b * B] for the nb = ceil(n / B) blocks of B strings, and reads the offsets of ONE block per batch.
#pragma once
#include <cstdint>
#include <algorithm>

/* the default budget of a batch and the strings it may hold, from the free device memory at the time of the call.  An insert holds about
 * 100 bytes per string of the batch (the position arrays of both sides, START, SIZE, the insert list), its text, and grows both pool
 * sides by less than a byte per symbol.  A sixteenth of what is free for the text (at most 4 GiB: the gain of larger batches is gone
 * long before) and a quarter of it for the per-string state (128 bytes each) leave more than half for the pools. */
static const int64_t MERGE_BUDGET_MIN = (int64_t)1 << 20, MERGE_BUDGET_MAX = (int64_t)1 << 32, MERGE_STRING_BYTES = 128;

inline int64_t merge_default_budget(int64_t free_bytes)
{
	return std::min(std::max(free_bytes / 16, MERGE_BUDGET_MIN), MERGE_BUDGET_MAX);
}

/* hard: the strings one batch of the engine may hold at the most (2^32 - 1024, or what RB2_MAX_BATCH_STRINGS says) */
inline int64_t merge_string_cap(int64_t free_bytes, int64_t hard)
{
	return std::max<int64_t>(1, std::min(hard, std::max(free_bytes / 4 / MERGE_STRING_BYTES, MERGE_BUDGET_MIN)));
}

struct MergeCut { int64_t end; uint64_t off_end; };    /* the batch is the strings [i0, end), its text off[i0] .. off_end */

/* The end of the batch that begins with string i0 (i0 < n, off0 = off[i0]): the largest end in (i0, min(n, i0 + max_strings)] with
 * off[end] - off0 <= budget, and i0 + 1 when there is none -- a single string longer than the budget is a batch of its own.
 * fetch(b, buf) fills buf[0 .. min(B, n - b * B)) with off[b * B ..]: the offsets of block b.  buf: room for B values.
 * max_strings >= 1; budget >= 0 (a budget of 0 gives one string per batch, as 1 does for empty strings). */
template <typename Fetch>
inline MergeCut merge_next_cut(const uint64_t *bsum, int64_t nb, int64_t n, uint64_t total, int64_t B, int64_t i0, uint64_t off0, uint64_t budget, int64_t max_strings,
                               uint64_t *buf, Fetch fetch)
{
	const uint64_t limit = budget > ~0ull - off0 ? ~0ull : off0 + budget;
	const int64_t hi = max_strings < n - i0 ? i0 + max_strings : n;          /* the last end allowed */
	int64_t lo_b = i0 / B, hi_b = std::min(hi / B, nb - 1);                 /* the last block whose first offset is within the limit: bsum[i0 / B] <= off0 always is */
	while (lo_b < hi_b) {
		const int64_t mid = lo_b + (hi_b - lo_b + 1) / 2;
		if (bsum[mid] <= limit) lo_b = mid; else hi_b = mid - 1;
	}
	const int64_t b = lo_b, e0 = b * B, cnt = std::min(B, n - e0);
	fetch(b, buf);
	auto at = [&](int64_t e) { return e - e0 < cnt ? buf[e - e0] : b + 1 < nb ? bsum[b + 1] : total; };   /* off[e] for e0 <= e <= e0 + cnt */
	int64_t lo = std::max(i0 + 1, e0), top = std::min(hi, e0 + cnt);        /* the candidates of this block: lo .. top */
	if (at(lo) > limit) return {lo, at(lo)};                                /* (lo == i0 + 1 then: off[e0] = bsum[b] is within the limit) the oversized string */
	while (lo < top) {
		const int64_t mid = lo + (top - lo + 1) / 2;
		if (at(mid) <= limit) lo = mid; else top = mid - 1;
	}
	return {lo, at(lo)};
}
