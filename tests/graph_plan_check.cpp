// CPU check of csrc/rb2_graph_plan.h (tests/test_graph_plan.py): the chunk cutter of rb2_hip_string_graph, driven as the host drives it --
// try, measure, cut, take -- over strings whose lengths only this program knows, against brute force.  A program of its own: prints
// "GRAPH PLAN OK cases <n> chunks <m>" and returns 0, or says what differs and returns 1.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "rb2_graph_plan.h"

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }

static long g_chunks = 0;

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } while (0)

// every chunk of the strings with these lengths (symbols, without the closing 0) under (chunk, max_recs, budget): returns the chunks.
// The offsets of a try count from any base, as the device's do from 0 for each try
static int64_t check(const std::vector<uint64_t> &len, int64_t chunk, int64_t max_recs, uint64_t budget, int64_t want_chunks, const char *what)
{
	const int64_t n = (int64_t)len.size(), limit = graph_chunk_limit(chunk, max_recs);
	if (limit < 1 || limit > chunk || (limit > 1 && limit * max_recs * 32 > GRAPH_REC_BYTES)) FAIL("%s: limit %lld for chunk %lld, max_recs %lld", what, (long long)limit, (long long)chunk, (long long)max_recs);
	if (limit < chunk && (limit + 1) * max_recs * 32 <= GRAPH_REC_BYTES) FAIL("%s: limit %lld is not the most the records allow", what, (long long)limit);
	GraphPlan p = graph_plan(chunk, max_recs);
	std::vector<int> seen((size_t)n, 0);
	int64_t i0 = 0, chunks = 0, measured = 0;
	while (i0 < n) {
		const int64_t tried = graph_try(p, n - i0);
		if (tried < 1 || tried > limit || tried > n - i0) FAIL("%s: %lld strings tried at %lld of %lld, limit %lld", what, (long long)tried, (long long)i0, (long long)n, (long long)limit);
		std::vector<uint64_t> off((size_t)tried + 1);                 // exactly tried + 1 values: a read behind them is the sanitizer's to find
		off[0] = rnd() % 1000;
		for (int64_t k = 0; k < tried; ++k) off[(size_t)k + 1] = off[(size_t)k] + len[(size_t)(i0 + k)] + 1;
		measured += tried;
		const int64_t took = graph_text_cut(off.data(), tried, budget);
		int64_t e = 1;                                                 // brute force: the oversized string alone, else as many as fit
		while (e < tried && off[(size_t)e + 1] - off[0] <= budget) ++e;
		if (took != e) FAIL("%s: the chunk at %lld took %lld of %lld tried, brute force %lld", what, (long long)i0, (long long)took, (long long)tried, (long long)e);
		if (off[(size_t)took] - off[0] > budget && took != 1) FAIL("%s: a chunk of several strings over the text budget", what);
		for (int64_t k = 0; k < took; ++k) ++seen[(size_t)(i0 + k)];
		graph_took(p, tried, took);
		if (p.next < 1 || p.next > limit) FAIL("%s: the next try is %lld, limit %lld", what, (long long)p.next, (long long)limit);
		i0 += took; ++chunks; ++g_chunks;
	}
	for (int64_t i = 0; i < n; ++i) if (seen[(size_t)i] != 1) FAIL("%s: string %lld is in %d chunks", what, (long long)i, seen[(size_t)i]);
	if (want_chunks >= 0 && chunks != want_chunks) FAIL("%s: %lld chunks, expected %lld", what, (long long)chunks, (long long)want_chunks);
	// what is measured and not taken: all of the first try at the most (n), a quarter of the chunk before plus one behind a cut, twice the chunk before behind a whole one
	if (measured > 4 * n + 2 * chunks) FAIL("%s: %lld strings measured for %lld strings in %lld chunks", what, (long long)measured, (long long)n, (long long)chunks);
	return chunks;
}

int main()
{
	long cases = 0;
	const int64_t NOLIM = (int64_t)1 << 24, R1 = GRAPH_REC_BYTES / 32;                            // R1: the max_recs at which one string's records fill the budget
	const uint64_t BIG = (uint64_t)GRAPH_TEXT_BYTES;
	std::vector<uint64_t> u = {4, 0, 9, 9, 1, 0, 0, 30, 2, 5, 5, 5, 0};                           // 13 strings, 83 bytes
	check(u, NOLIM, 16, BIG, 1, "everything in one chunk"); ++cases;
	check(u, NOLIM, 16, 83, 1, "the whole text exactly"); ++cases;
	check(u, NOLIM, 16, 82, 2, "the whole text minus 1"); ++cases;
	check(u, NOLIM, 16, 1, 13, "a text budget of 1"); ++cases;
	check(u, NOLIM, 16, 0, 13, "a text budget of 0"); ++cases;
	check(u, 1, 16, BIG, 13, "a chunk of 1 string"); ++cases;
	check(u, 3, 16, BIG, 5, "chunks of 3 strings"); ++cases;
	check(u, 13, 16, BIG, 1, "a chunk of all strings"); ++cases;
	check(u, NOLIM, R1 / 3, BIG, 5, "records for 3 strings"); ++cases;
	check(u, NOLIM, R1, BIG, 13, "records for one string exactly"); ++cases;
	check(u, NOLIM, R1 + 1, BIG, 13, "a record budget below one string's"); ++cases;
	check(u, NOLIM, INT64_MAX / 64, BIG, 13, "max_recs near the top of its type"); ++cases;
	check(u, 2, R1 / 3, BIG, 7, "the string limit before the records"); ++cases;
	std::vector<uint64_t> f = {99, 1, 1, 1, 1}, l = {1, 1, 1, 1, 99}, a = {99}, z(37, 0);
	check(f, NOLIM, 16, 4, 3, "an oversized string first"); ++cases;
	check(l, NOLIM, 16, 4, 3, "an oversized string last"); ++cases;
	check(a, NOLIM, 16, 4, 1, "an oversized string alone"); ++cases;
	check(a, NOLIM, 16, 100, 1, "a single string that fits"); ++cases;
	check(z, NOLIM, 16, 5, 8, "all-empty strings, a budget of 5"); ++cases;
	check(z, 5, 16, 1000, 8, "all-empty strings, the string limit first"); ++cases;
	for (int t = 0; t < 4000; ++t) {                                                               // random lengths, budgets and limits
		const int64_t n = 1 + (int64_t)(rnd() % 300);
		std::vector<uint64_t> len((size_t)n);
		const uint64_t top = 1 + rnd() % 60;
		for (auto &v : len) v = rnd() % 8 == 0 ? rnd() % 2000 : rnd() % top;
		const uint64_t budget = rnd() % 4 == 0 ? rnd() % 5 : rnd() % 3000;
		const int64_t chunk = rnd() % 3 == 0 ? 1 + (int64_t)(rnd() % 50) : NOLIM;
		const int64_t recs = rnd() % 3 == 0 ? R1 / (1 + (int64_t)(rnd() % 40)) : 16;
		check(len, chunk, recs, budget, -1, "random"); ++cases;
	}
	printf("GRAPH PLAN OK cases %ld chunks %ld\n", cases, g_chunks);
	return 0;
}
