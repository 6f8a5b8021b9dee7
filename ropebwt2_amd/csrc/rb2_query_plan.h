// How the host side of the FM-index queries (rb2_query_host.h) cuts its work into launches: the arithmetic alone, plain C++ with no
// HIP in it, so that a CPU program can include it (tests/test_query_plan.py).
#pragma once
#include <algorithm>
#include <cstdint>

/* what a host variant stages on the device for one launch: the records (or extracted strings) of a chunk stay under this */
static const int64_t QUERY_STAGE_BYTES = (int64_t)256 << 20;

/* items per launch of a host variant: at most chunk, as many as QUERY_STAGE_BYTES hold at bytes_per_item (> 0) each, one at the least */
static inline int64_t record_chunk(int64_t chunk, int64_t bytes_per_item)
{
	return std::max<int64_t>(1, std::min(chunk, QUERY_STAGE_BYTES / bytes_per_item));
}

/* n items of max_hits (>= 1) slots each in launches of at most launch_cap (>= 1) slots: f(i0, nc, k0, kc) takes the slots [k0, k0 + kc) of
 * the items [i0, i0 + nc), in increasing (i0, k0) -- whole items, or a part of the slots of one item when max_hits alone is larger than
 * a launch */
template <typename F> static inline void split_slots(int64_t n, int64_t max_hits, int64_t launch_cap, F f)
{
	const int64_t kn = std::min(max_hits, launch_cap), per = std::max<int64_t>(1, launch_cap / kn);
	for (int64_t i0 = 0; i0 < n; i0 += per)
		for (int64_t k0 = 0; k0 < max_hits; k0 += kn) f(i0, std::min(per, n - i0), k0, std::min(kn, max_hits - k0));
}
