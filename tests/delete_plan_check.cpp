// Brute-force check of csrc/rb2_delete_plan.h, the bit arithmetic of string deletion that needs no GPU.  Built and run by
// tests/test_delete_plan.py, once plain and once under AddressSanitizer + UndefinedBehaviorSanitizer; prints "DELETE PLAN OK" and leaves
// with 0 when every property holds.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "rb2_delete_plan.h"

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "%s:%d: %s failed: ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

// the bits of x under m, packed to the low end, one bit at a time
static uint64_t compress_loop(uint64_t x, uint64_t m)
{
	uint64_t r = 0;
	int k = 0;
	for (int i = 0; i < 64; ++i)
		if (m >> i & 1) { r |= (x >> i & 1) << k; ++k; }
	return r;
}

static long n_masks = 0;
static void check_mask(uint64_t m)
{
	const DelCompress P = del_compress_plan(m);
	const uint64_t xs[6] = { ~0ull, m, ~m, rnd(), rnd(), rnd() & rnd() };
	for (uint64_t x : xs) {
		const uint64_t got = del_compress(P, x), want = compress_loop(x, m);
		CHECK(got == want, "mask %016llx, word %016llx: compress gives %016llx, the loop %016llx", (unsigned long long)m, (unsigned long long)x, (unsigned long long)got, (unsigned long long)want);
	}
	const int c = __builtin_popcountll(m);
	CHECK(del_compress(P, ~0ull) == (c == 64 ? ~0ull : (1ull << c) - 1), "mask %016llx: the kept bits are not the low %d", (unsigned long long)m, c);
	bool prefix = true;                                        // the set bits are the low ones
	for (int i = 0; i < 64; ++i) if ((m >> i & 1) != (uint64_t)(i < c)) prefix = false;
	CHECK(del_mask_is_prefix(m) == prefix, "mask %016llx: prefix test", (unsigned long long)m);
	if (prefix) for (uint64_t x : xs) CHECK((x & m) == compress_loop(x, m), "mask %016llx: the fast path is not the compress", (unsigned long long)m);
	++n_masks;
}

static void check_compress()
{
	check_mask(0); check_mask(~0ull); check_mask(0x5555555555555555ull); check_mask(0xaaaaaaaaaaaaaaaaull);
	for (int i = 0; i < 64; ++i) {                             // at most two set bits, at most two clear bits
		check_mask(1ull << i); check_mask(~(1ull << i));
		for (int j = i + 1; j < 64; ++j) { check_mask(1ull << i | 1ull << j); check_mask(~(1ull << i | 1ull << j)); }
	}
	for (int t = 0; t < 100000; ++t) {
		uint64_t m = rnd();
		if (t % 4 == 1) m &= rnd(); else if (t % 4 == 2) m |= rnd(); else if (t % 4 == 3) m = ~(rnd() & rnd() & rnd());   // sparse, dense, a few holes
		check_mask(m);
	}
}

// a destination piece of `leaves` leaves behind leaf0: c kept bits written at row d through del_dst against a model that places one
// symbol at a time
static long n_splits = 0;
static void check_split()
{
	const uint64_t leaf0 = 3, leaves = 3, words = (leaf0 + leaves) * DEL_LEAFW;
	std::vector<uint64_t> got(words), want(words);
	const uint64_t d0s[] = { 0, 64 * 7, 64 * 15, 1024 + 64 * 15, 1024 };   // a first group, a middle one, a leaf's last group (twice), a leaf's first
	for (uint64_t d0 : d0s)
		for (uint32_t sh = 0; sh < 64; ++sh)
			for (uint32_t c = 0; c <= 64; ++c)
				for (uint32_t pl = 0; pl < 3; ++pl) {
					const uint64_t d = d0 + sh, bits = c == 64 ? ~0ull : ((1ull << c) - 1);   // every kept bit set: what lands where
					std::fill(got.begin(), got.end(), 0); std::fill(want.begin(), want.end(), 0);
					const DelDst D = del_dst(leaf0, d, c, pl);
					CHECK(D.shift == sh, "shift");
					CHECK(D.word < words, "word %llu outside the piece", (unsigned long long)D.word);
					got[D.word] |= bits << D.shift;
					if (D.spill) {
						CHECK(D.shift > 0 && D.word2 < words, "spill word %llu outside the piece", (unsigned long long)D.word2);
						got[D.word2] |= bits >> (64 - D.shift);
					} else CHECK(D.shift == 0 || (bits >> (64 - D.shift)) == 0, "bits lost: d %llu c %u", (unsigned long long)d, c);
					for (uint32_t k = 0; k < c; ++k) {                 // symbol k goes to row d + k: leaf, group and bit of that row
						const uint64_t row = d + k, leaf = leaf0 + row / 1024, g = row / 64 % 16;
						want[leaf * 48 + pl * 16 + g] |= 1ull << (row % 64);
					}
					CHECK(got == want, "d %llu, c %u, plane %u: the split differs from the model", (unsigned long long)d, c, pl);
					if (c > 0) CHECK(D.word == (leaf0 + d / 1024) * 48 + pl * 16 + d / 64 % 16, "word");
					if (D.spill) CHECK(D.word2 == (leaf0 + (d + 64 - sh) / 1024) * 48 + pl * 16 + (d + 64 - sh) / 64 % 16, "spill word");
					++n_splits;
				}
	// the group behind a leaf's last one is the first of the next leaf
	CHECK(del_dst(0, 64 * 15 + 1, 64, 2).word2 == 48 + 2 * 16, "the spill of a leaf's last group");
}

int main()
{
	check_compress();
	check_split();
	printf("DELETE PLAN OK masks %ld splits %ld\n", n_masks, n_splits);
	return 0;
}
