// CPU check of csrc/rb2_merge_plan.h (tests/test_merge_plan.py): the batch cutter against brute force over the whole offset array, and
// the default budget.  A program of its own: prints "MERGE PLAN OK cases <n> cuts <m>" and returns 0, or says what differs and returns 1.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "rb2_merge_plan.h"

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }

static long g_cuts = 0, g_fetches = 0;

// every batch of the strings with these lengths (symbols, without the 0) under (budget, max_strings), block size B: returns the batches
static int check(const std::vector<uint64_t> &len, int64_t B, uint64_t budget, int64_t max_strings, int64_t want_batches, const char *what)
{
	const int64_t n = (int64_t)len.size(), nb = (n + B - 1) / B;
	std::vector<uint64_t> off((size_t)n + 1, 0), bsum((size_t)nb), buf((size_t)B);
	for (int64_t i = 0; i < n; ++i) off[(size_t)i + 1] = off[(size_t)i] + len[(size_t)i] + 1;
	for (int64_t b = 0; b < nb; ++b) bsum[(size_t)b] = off[(size_t)(b * B)];
	int64_t i0 = 0, batches = 0;
	uint64_t off0 = 0;
	while (i0 < n) {
		int fetched = 0;
		const MergeCut c = merge_next_cut(bsum.data(), nb, n, off[(size_t)n], B, i0, off0, budget, max_strings, buf.data(), [&](int64_t b, uint64_t *o) {
			++fetched; ++g_fetches;
			if (b < 0 || b >= nb) { fprintf(stderr, "%s: block %lld of %lld fetched\n", what, (long long)b, (long long)nb); exit(1); }
			for (int64_t k = 0; k < B && b * B + k < n; ++k) o[k] = off[(size_t)(b * B + k)]; });
		int64_t e = i0 + 1;                                            // brute force: the oversized string alone, else as many as fit
		while (e < n && e - i0 < max_strings && off[(size_t)e + 1] - off0 <= budget) ++e;
		if (fetched != 1 || c.end != e || c.off_end != off[(size_t)e]) {
			fprintf(stderr, "%s: n %lld B %lld budget %llu max %lld i0 %lld: end %lld off %llu (%d fetches), brute force %lld off %llu\n", what, (long long)n, (long long)B,
					(unsigned long long)budget, (long long)max_strings, (long long)i0, (long long)c.end, (unsigned long long)c.off_end, fetched, (long long)e, (unsigned long long)off[(size_t)e]);
			exit(1);
		}
		const uint64_t bytes = c.off_end - off0;
		if (bytes > budget && c.end != i0 + 1) { fprintf(stderr, "%s: a batch of several strings over the budget\n", what); exit(1); }
		i0 = c.end; off0 = c.off_end; ++batches; ++g_cuts;
	}
	if (want_batches >= 0 && batches != want_batches) { fprintf(stderr, "%s: %lld batches, expected %lld\n", what, (long long)batches, (long long)want_batches); exit(1); }
	return (int)batches;
}

int main()
{
	long cases = 0;
	const int64_t NOLIM = (int64_t)1 << 40;
	for (int64_t B : {1, 2, 3, 4, 7, 16, 4096}) {
		std::vector<uint64_t> u = {4, 0, 9, 9, 1, 0, 0, 30, 2, 5, 5, 5, 0};                        // 13 strings, 83 bytes
		check(u, B, 1, NOLIM, 13, "a budget of 1"); ++cases;                                        // (every string is oversized or exactly one byte)
		check(u, B, 0, NOLIM, 13, "a budget of 0"); ++cases;
		check(u, B, 83, NOLIM, 1, "the whole text"); ++cases;
		check(u, B, 82, NOLIM, 2, "the whole text minus 1"); ++cases;
		check(u, B, ~0ull, NOLIM, 1, "no budget to speak of"); ++cases;
		std::vector<uint64_t> s(10, 9);                                                            // ten strings of 10 bytes
		check(s, B, 10, NOLIM, 10, "one string exactly"); ++cases;
		check(s, B, 9, NOLIM, 10, "one string minus 1"); ++cases;
		check(s, B, 20, NOLIM, 5, "two strings exactly"); ++cases;
		check(s, B, 19, NOLIM, 10, "two strings minus 1"); ++cases;
		check(s, B, 29, NOLIM, 5, "two strings and a rest"); ++cases;
		std::vector<uint64_t> f = {99, 1, 1, 1, 1}, l = {1, 1, 1, 1, 99}, a = {99};
		check(f, B, 4, NOLIM, 3, "an oversized string first"); ++cases;
		check(l, B, 4, NOLIM, 3, "an oversized string last"); ++cases;
		check(a, B, 4, NOLIM, 1, "an oversized string alone"); ++cases;
		check(a, B, 100, NOLIM, 1, "a single string that fits"); ++cases;
		std::vector<uint64_t> z(37, 0);
		check(z, B, 1, NOLIM, 37, "all-empty strings, a budget of 1"); ++cases;
		check(z, B, 5, NOLIM, 8, "all-empty strings, a budget of 5"); ++cases;
		check(z, B, 1000, NOLIM, 1, "all-empty strings, one batch"); ++cases;
		check(z, B, 1000, 5, 8, "the string limit before the byte budget"); ++cases;
		check(z, B, 1000, 1, 37, "a string limit of 1"); ++cases;
		check(z, B, 1000, 37, 1, "a string limit of all"); ++cases;
		check(s, B, 35, 2, 5, "the string limit and the budget in turn"); ++cases;
	}
	for (int t = 0; t < 4000; ++t) {                                                               // random lengths, budgets, limits and block sizes
		const int64_t n = 1 + (int64_t)(rnd() % 300), B = 1 + (int64_t)(rnd() % 40);
		std::vector<uint64_t> len((size_t)n);
		const uint64_t top = 1 + rnd() % 60;
		for (auto &v : len) v = rnd() % 8 == 0 ? rnd() % 2000 : rnd() % top;
		const uint64_t budget = rnd() % 4 == 0 ? rnd() % 5 : rnd() % 3000;
		const int64_t mx = rnd() % 3 == 0 ? 1 + (int64_t)(rnd() % 50) : NOLIM;
		check(len, B, budget, mx, -1, "random"); ++cases;
	}
	// the default budget: a sixteenth of what is free inside [1 MiB, 4 GiB]; strings: a quarter of it at 128 bytes, at least 2^20, at most the engine's limit
	const int64_t G = (int64_t)1 << 30, hard = ((int64_t)1 << 32) - 1025;
	if (merge_default_budget(0) != 1 << 20 || merge_default_budget(16 * G) != G || merge_default_budget(288 * G) != 4 * G || merge_default_budget(32 << 20) != 2 << 20) { fprintf(stderr, "default budget\n"); return 1; }
	if (merge_string_cap(0, hard) != 1 << 20 || merge_string_cap(64 * G, hard) != 64 * G / 512 || merge_string_cap((int64_t)1 << 50, hard) != hard || merge_string_cap(G, 7) != 7 || merge_string_cap(G, 0) != 1) { fprintf(stderr, "string cap\n"); return 1; }
	if (g_fetches != g_cuts) { fprintf(stderr, "%ld fetches for %ld cuts\n", g_fetches, g_cuts); return 1; }
	printf("MERGE PLAN OK cases %ld cuts %ld\n", cases, g_cuts);
	return 0;
}
