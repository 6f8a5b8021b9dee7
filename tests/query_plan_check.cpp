// Brute-force check of csrc/rb2_query_plan.h, the launch arithmetic of the query host layer.  Built and run by tests/test_query_plan.py
// under AddressSanitizer + UndefinedBehaviorSanitizer; prints "PLAN OK" and leaves with 0 when every property holds.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "rb2_query_plan.h"

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "%s:%d: %s failed: ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

struct Call { int64_t i0, nc, k0, kc; };

static long check_split()
{
	const int64_t caps[] = {1, 2, 3, 5, 8, 16, 64};
	long calls_seen = 0, partial = 0;
	for (int64_t n = 0; n <= 9; ++n)
		for (int64_t max_hits = 1; max_hits <= 20; ++max_hits)
			for (int64_t cap : caps) {
				std::vector<Call> calls;
				split_slots(n, max_hits, cap, [&](int64_t i0, int64_t nc, int64_t k0, int64_t kc) { calls.push_back({i0, nc, k0, kc}); });
				std::vector<int> seen((size_t)(n * max_hits), 0);
				for (size_t c = 0; c < calls.size(); ++c) {
					const Call &a = calls[c];
					CHECK(a.nc >= 1 && a.kc >= 1 && a.i0 >= 0 && a.k0 >= 0 && a.i0 + a.nc <= n && a.k0 + a.kc <= max_hits,
					      "n %lld max_hits %lld cap %lld: call (%lld, %lld, %lld, %lld) leaves the slots", (long long)n, (long long)max_hits, (long long)cap,
					      (long long)a.i0, (long long)a.nc, (long long)a.k0, (long long)a.kc);
					CHECK(a.nc * a.kc <= std::max<int64_t>(cap, 1), "n %lld max_hits %lld cap %lld: a call of %lld slots", (long long)n, (long long)max_hits, (long long)cap,
					      (long long)(a.nc * a.kc));
					if (c) CHECK(calls[c - 1].i0 < a.i0 || (calls[c - 1].i0 == a.i0 && calls[c - 1].k0 < a.k0), "n %lld max_hits %lld cap %lld: call %zu is out of order",
					             (long long)n, (long long)max_hits, (long long)cap, c);
					for (int64_t i = a.i0; i < a.i0 + a.nc; ++i)
						for (int64_t k = a.k0; k < a.k0 + a.kc; ++k) ++seen[(size_t)(i * max_hits + k)];
					partial += a.kc < max_hits;
				}
				for (int64_t s = 0; s < n * max_hits; ++s)
					CHECK(seen[(size_t)s] == 1, "n %lld max_hits %lld cap %lld: slot (%lld, %lld) is covered %d times", (long long)n, (long long)max_hits, (long long)cap,
					      (long long)(s / max_hits), (long long)(s % max_hits), seen[(size_t)s]);
				if (n && cap >= n * max_hits) CHECK(calls.size() == 1, "n %lld max_hits %lld cap %lld: %zu calls where one launch holds everything", (long long)n,
				                                    (long long)max_hits, (long long)cap, calls.size());
				if (!n) CHECK(calls.empty(), "max_hits %lld cap %lld: %zu calls for no items", (long long)max_hits, (long long)cap, calls.size());
				calls_seen += (long)calls.size();
			}
	CHECK(partial > 0, "no case split the slots of one item");       // caps below max_hits: the branch the engine's own caps never reach at a test size
	return calls_seen;
}

static void check_record_chunk()
{
	const int64_t B = (int64_t)256 << 20;                             // the budget as the five expressions spelled it before they were one function
	CHECK(QUERY_STAGE_BYTES == B, "the staging budget is %lld", (long long)QUERY_STAGE_BYTES);
	const int64_t chunks[] = {1, 7, (int64_t)1 << 24}, caps[] = {1, 64, (int64_t)1 << 20, (int64_t)1 << 31};
	for (int64_t chunk : chunks)
		for (int64_t m : caps) {
			const int64_t old_smem = std::max<int64_t>(1, std::min<int64_t>(chunk, B / 40 / m)), old_locate = std::max<int64_t>(1, std::min<int64_t>(chunk, B / 16 / m)),
			              old_overlap = std::max<int64_t>(1, std::min<int64_t>(chunk, B / 24 / m)), old_ids = std::max<int64_t>(1, std::min<int64_t>(chunk, B / 8 / m)),
			              old_extract = std::max<int64_t>(1, std::min<int64_t>(chunk, (int64_t)(256u << 20) / m));
			CHECK(record_chunk(chunk, 40 * m) == old_smem, "smem: chunk %lld max_mems %lld", (long long)chunk, (long long)m);
			CHECK(record_chunk(chunk, 16 * m) == old_locate, "locate: chunk %lld max_hits %lld", (long long)chunk, (long long)m);
			CHECK(record_chunk(chunk, 24 * m) == old_overlap, "overlap: chunk %lld max_recs %lld", (long long)chunk, (long long)m);
			CHECK(record_chunk(chunk, 8 * m) == old_ids, "string_ids: chunk %lld max_hits %lld", (long long)chunk, (long long)m);
			CHECK(record_chunk(chunk, m) == old_extract, "extract: chunk %lld max_len %lld", (long long)chunk, (long long)m);
		}
	const int64_t sizes[] = {1, 2, 3, 8, 40, 1000, 4097, B / 3, B / 2, B / 2 + 1, B - 1, B, B + 1, 2 * B, (int64_t)40 << 31, INT64_MAX};
	const int64_t more_chunks[] = {1, 2, 7, 1000, (int64_t)1 << 24, INT64_MAX};
	for (int64_t chunk : more_chunks)
		for (int64_t b : sizes) {
			const int64_t r = record_chunk(chunk, b);
			CHECK(r >= 1 && r <= chunk, "record_chunk(%lld, %lld) = %lld", (long long)chunk, (long long)b, (long long)r);
			if (b <= B) CHECK(r <= B / b && r * b <= B, "record_chunk(%lld, %lld) = %lld is over the budget", (long long)chunk, (long long)b, (long long)r);
			else CHECK(r == 1, "record_chunk(%lld, %lld) = %lld for an item larger than the budget", (long long)chunk, (long long)b, (long long)r);
			if (b <= B) CHECK(r == chunk || (r + 1) * b > B, "record_chunk(%lld, %lld) = %lld leaves room for another item", (long long)chunk, (long long)b, (long long)r);
		}
}

int main()
{
	const long calls = check_split();
	check_record_chunk();
	printf("PLAN OK %ld calls\n", calls);
	return 0;
}
