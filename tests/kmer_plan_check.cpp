// Brute-force check of csrc/rb2_kmer_plan.h, the arithmetic of the k-mer enumeration that needs no GPU.  Built and run by
// tests/test_kmer_plan.py, once plain and once under AddressSanitizer + UndefinedBehaviorSanitizer; prints "KMER PLAN OK" and leaves with 0
// when every property holds.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "rb2_kmer_plan.h"

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "%s:%d: %s failed: ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

// pack, unpack and reverse complement, symbol by symbol, for every k
static long check_codes()
{
	long n = 0;
	for (int k = 1; k <= KMER_MAX_K; ++k)
		for (int t = 0; t < 200; ++t) {
			int s[KMER_MAX_K], rc[KMER_MAX_K];
			for (int p = 0; p < k; ++p) s[p] = t == 0 ? 1 : t == 1 ? 4 : 1 + (int)(rnd() % 4);
			uint64_t code = 0, want = 0, rcode = 0;
			for (int p = k - 1, l = 0; p >= 0; --p, ++l) code = kmer_prepend(code, l, s[p]);      // built as the walk builds it: last symbol first
			for (int p = 0; p < k; ++p) want = want << 2 | (uint64_t)(s[p] - 1);
			CHECK(code == want, "k %d: prepend gives %llx, the definition %llx", k, (unsigned long long)code, (unsigned long long)want);
			for (int p = 0; p < k; ++p) CHECK(kmer_symbol(code, k, p) == s[p], "k %d: symbol %d", k, p);
			for (int p = 0; p < k; ++p) rc[p] = 5 - s[k - 1 - p];
			for (int p = 0; p < k; ++p) rcode = rcode << 2 | (uint64_t)(rc[p] - 1);
			CHECK(kmer_revcomp(code, k) == rcode, "k %d: revcomp(%llx) = %llx, want %llx", k, (unsigned long long)code, (unsigned long long)kmer_revcomp(code, k), (unsigned long long)rcode);
			CHECK(kmer_revcomp(rcode, k) == code, "k %d: revcomp is no involution", k);
			CHECK(kmer_canonical(code, k) == (code <= rcode) && (kmer_canonical(code, k) || kmer_canonical(rcode, k)), "k %d: canonical", k);
			if (k % 2 == 0) {                                       // a palindrome: the second half is the reverse complement of the first
				for (int p = 0; p < k / 2; ++p) s[k - 1 - p] = 5 - s[p];
				uint64_t pal = 0;
				for (int p = 0; p < k; ++p) pal = pal << 2 | (uint64_t)(s[p] - 1);
				CHECK(kmer_revcomp(pal, k) == pal && kmer_canonical(pal, k), "k %d: palindrome %llx", k, (unsigned long long)pal);
			}
			++n;
		}
	uint64_t x = 0x0123456789abcdefull, r = 0;
	for (int i = 0; i < 32; ++i) r |= (x >> (2 * i) & 3) << (2 * (31 - i));
	CHECK(kmer_rev2(x) == r, "rev2");
	return n;
}

// slices: a segment is emptied in slices of at most F / 4 items, at least one, and the children of a slice fit the next segment
static long check_slices()
{
	long n = 0;
	const int64_t Fs[] = {4, 5, 7, 8, 63, 64, 1000, (int64_t)1 << 22, (int64_t)1 << 40};
	for (int64_t F : Fs) {
		CHECK(F >= KMER_FRONTIER_MIN, "F");
		for (int64_t avail = 1; avail <= 300; avail += (avail < 40 ? 1 : 37)) {
			int64_t left = avail, slices = 0;
			while (left > 0) {
				const int64_t t = kmer_slice(left, F);
				CHECK(t >= 1 && t <= left && 4 * t <= F, "F %lld avail %lld: slice %lld", (long long)F, (long long)left, (long long)t);
				CHECK(t == left || 4 * (t + 1) > F, "F %lld avail %lld: slice %lld could be larger", (long long)F, (long long)left, (long long)t);
				left -= t; ++slices; ++n;
			}
			CHECK(slices == (avail + F / 4 - 1) / (F / 4), "F %lld avail %lld: %lld slices", (long long)F, (long long)avail, (long long)slices);
		}
		const int64_t Ns[] = {1, 3, 4, 5, 1000, (int64_t)1 << 33, (int64_t)1 << 62};
		for (int64_t N : Ns)
			for (int l = 0; l <= KMER_MAX_K; ++l) {
				const int64_t c = kmer_segment_cap(l, F, N);
				int64_t p4 = 1;                                     // min(4^l, 2^62), without overflow
				for (int q = 0; q < l && p4 < ((int64_t)1 << 62); ++q) p4 *= 4;
				CHECK(c == std::min(std::min(F, N), p4), "cap(l %d, F %lld, N %lld) = %lld", l, (long long)F, (long long)N, (long long)c);
				if (l > 0) {                                        // the children of the largest slice of level l - 1 fit
					const int64_t parent = kmer_segment_cap(l - 1, F, N), most = std::min(std::min(4 * kmer_slice(parent, F), N), p4);
					CHECK(most <= c, "l %d F %lld N %lld: %lld children, a segment of %lld", l, (long long)F, (long long)N, (long long)most, (long long)c);
				}
				++n;
			}
	}
	return n;
}

// the record staging: a simulated walk draws numbers as the device cursor does; every number below max_recs must land in exactly one
// slot inside the staging buffer and reach the caller's array exactly once, whatever the flushes
static long check_staging()
{
	long n = 0, flushes = 0, limited = 0;
	const int64_t limits[] = {4, 5, 9, 16, 100, (int64_t)1 << 30}, maxes[] = {0, 1, 3, 4, 17, 100, 1000}, Fs[] = {4, 8, 64, 1000};
	for (int64_t limit : limits)
		for (int64_t max_recs : maxes)
			for (int64_t F : Fs)
				for (int round = 0; round < 4; ++round) {
					const int64_t stage = kmer_stage_recs(max_recs, limit);
					CHECK(stage == std::min(max_recs, limit), "stage");
					std::vector<int64_t> buf((size_t)stage, -1), rec((size_t)max_recs, -1);
					int64_t found = 0, flushed = 0;
					auto flush = [&]() {
						const int64_t m = kmer_staged(found, flushed, max_recs);
						CHECK(m >= 0 && m <= stage, "limit %lld max_recs %lld: a flush of %lld records", (long long)limit, (long long)max_recs, (long long)m);
						for (int64_t q = 0; q < m; ++q) { CHECK(rec[(size_t)(flushed + q)] == -1, "a record is delivered twice"); rec[(size_t)(flushed + q)] = buf[(size_t)q]; buf[(size_t)q] = -1; }
						flushed += m;
					};
					for (int seg = 0; seg < 6; ++seg) {
						int64_t avail = 1 + (int64_t)(rnd() % (uint64_t)F);
						while (avail > 0) {
							const int64_t take = kmer_final_slice(avail, F, stage, max_recs);
							CHECK(take >= 1 && take <= avail && take <= kmer_slice(avail, F), "final slice %lld of %lld", (long long)take, (long long)avail);
							limited += take < kmer_slice(avail, F);
							avail -= take;
							if (kmer_must_flush(found, flushed, take, stage, max_recs)) { flush(); ++flushes; }
							const int64_t kids = round == 0 ? 4 * take : (int64_t)(rnd() % (uint64_t)(4 * take + 1));
							for (int64_t q = 0; q < kids; ++q) {          // what k_kmer_expand does with number j
								const int64_t j = found++;
								if (j < max_recs && j >= flushed && j - flushed < stage) { CHECK(buf[(size_t)(j - flushed)] == -1, "a slot is written twice"); buf[(size_t)(j - flushed)] = j; }
								else CHECK(j >= max_recs, "limit %lld max_recs %lld F %lld: number %lld has no slot (flushed %lld, stage %lld)", (long long)limit, (long long)max_recs,
								           (long long)F, (long long)j, (long long)flushed, (long long)stage);
							}
							++n;
						}
					}
					flush();
					for (int64_t j = 0; j < max_recs; ++j) CHECK(rec[(size_t)j] == (j < found ? j : -1), "max_recs %lld: record %lld holds %lld", (long long)max_recs, (long long)j, (long long)rec[(size_t)j]);
				}
	CHECK(flushes > 0 && limited > 0, "no case flushed (%ld) or limited a slice (%ld)", flushes, limited);
	return n;
}

int main()
{
	const long a = check_codes(), b = check_slices(), c = check_staging();
	printf("KMER PLAN OK %ld codes %ld slices %ld launches\n", a, b, c);
	return 0;
}
