// Brute-force check of the approximate-search part of csrc/rb2_query_plan.h, the arithmetic of rb2_hip_approx that needs no GPU: the rows
// and the stacks of a launch, the split of a call into a launch for the short and one for the long queries, the packing of the
// substitutions, and the piece bound against the true minimum of substitutions over tiny sets of strings.  Built and run by
// tests/test_approx_plan.py, once plain and once under AddressSanitizer + UndefinedBehaviorSanitizer; prints "APPROX PLAN OK" and leaves
// with 0 when every property holds.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>
#include "rb2_query_plan.h"

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "%s:%d: %s failed: ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

// rows, stacks and passes
static long check_launches()
{
	long n = 0, two = 0;
	CHECK(approx_row_bytes(1) == 80 && approx_row_bytes(8) == 528 && approx_row_bytes(101) == 64 * 101 + 208 && approx_row_bytes(APPROX_MAX_LEN) == 66 * APPROX_MAX_LEN, "row bytes");
	for (int64_t L = 1; L <= APPROX_MAX_LEN; ++L) {
		CHECK(approx_row_bytes(L) % 8 == 0 && approx_row_bytes(L) >= 66 * L && approx_pad(L) >= L && approx_pad(L) < L + 8, "L %lld", (long long)L);
		CHECK(L == 1 || approx_row_bytes(L) > approx_row_bytes(L - 1) - 16, "L %lld", (long long)L);
	}
	const int64_t sizes[] = {1, 79, 80, 81, 4096, 65536, 67584, 8650752, (int64_t)1 << 24, APPROX_SCRATCH_BYTES};
	const int64_t ns[] = {1, 2, 15, 16, 17, 300, 496, 497, 16383, 16384, 16385, 40000, 1 << 20, (int64_t)1 << 24};
	const int64_t lens[] = {1, 2, 7, 8, 9, 40, 101, 247, 248, 249, 1000, 8191, 8192};
	for (int64_t bytes : sizes) {
		for (int64_t rows : {(int64_t)1, (int64_t)16, (int64_t)496, APPROX_SHORT_ROWS, APPROX_ROWS}) {
			const int64_t c = stack_len_cap(rows, bytes, approx_row_bytes);
			CHECK(c >= 0 && c <= APPROX_MAX_LEN, "cap");
			CHECK(c == 0 || approx_row_bytes(c) * rows <= bytes, "rows %lld bytes %lld: cap %lld does not fit", (long long)rows, (long long)bytes, (long long)c);
			CHECK(c == APPROX_MAX_LEN || approx_row_bytes(c + 1) * rows > bytes, "rows %lld bytes %lld: cap %lld could be larger", (long long)rows, (long long)bytes, (long long)c);
			++n;
		}
		for (int64_t nq : ns)
			for (int64_t lmax : lens) {
				const int64_t r = stack_rows(nq, approx_row_bytes(lmax), bytes, APPROX_ROWS);
				CHECK(r >= 1 && r <= nq && r <= APPROX_ROWS, "rows");
				CHECK(r == 1 || r * approx_row_bytes(lmax) <= bytes, "n %lld L %lld bytes %lld: %lld rows do not fit", (long long)nq, (long long)lmax, (long long)bytes, (long long)r);
				CHECK(r == nq || r == APPROX_ROWS || (r + 1) * approx_row_bytes(lmax) > bytes, "n %lld L %lld bytes %lld: %lld rows could be more", (long long)nq, (long long)lmax, (long long)bytes, (long long)r);
				int64_t pass[2][4];
				const int np = stack_passes(nq, lmax, bytes, approx_row_bytes, pass);
				CHECK(np == 1 || np == 2, "passes");
				two += np == 2;
				for (int k = 0; k < np; ++k) {
					CHECK(pass[k][3] >= 1 && pass[k][3] <= nq && pass[k][3] <= APPROX_ROWS && pass[k][2] >= 1 && pass[k][2] <= lmax, "pass %d", k);
					CHECK(pass[k][3] == 1 || pass[k][3] * approx_row_bytes(pass[k][2]) <= bytes, "pass %d: the stacks do not fit", k);
				}
				const int64_t probe[] = {INT64_MIN, -5, -1, 0, 1, 2, 8, 9, 247, 248, 249, lmax - 1, lmax, lmax + 1, APPROX_MAX_LEN, APPROX_MAX_LEN + 1, INT64_MAX};
				for (int64_t L : probe) {                           // what k_approx asks: lmin < L <= lcap
					int owners = 0;
					for (int k = 0; k < np; ++k)
						if (L > pass[k][0] && L <= pass[k][1]) {
							++owners;
							CHECK(L > lmax || L <= pass[k][2], "n %lld lmax %lld bytes %lld: a query of %lld in a launch with stacks for %lld", (long long)nq, (long long)lmax, (long long)bytes, (long long)L, (long long)pass[k][2]);
						}
					CHECK(owners == 1 || (L == INT64_MIN && owners == 0), "n %lld lmax %lld bytes %lld: length %lld has %d launches", (long long)nq, (long long)lmax, (long long)bytes, (long long)L, owners);
				}
				if (np == 2) CHECK(pass[0][3] > pass[1][3] && pass[0][2] < pass[1][2], "the short launch must have more rows");
				++n;
			}
	}
	int64_t pass[2][4];
	CHECK(stack_passes(100000, APPROX_MAX_LEN, APPROX_SCRATCH_BYTES, approx_row_bytes, pass) == 2 && pass[0][1] == 248 && pass[0][3] >= APPROX_SHORT_ROWS && pass[0][3] < APPROX_SHORT_ROWS + 64 && pass[1][3] == 496, "the _dev variant: %lld %lld %lld",
	      (long long)pass[0][1], (long long)pass[0][3], (long long)pass[1][3]);
	CHECK(stack_passes(100000, 101, APPROX_SCRATCH_BYTES, approx_row_bytes, pass) == 1 && pass[0][3] == APPROX_ROWS, "reads of 101");
	CHECK(stack_passes(400, APPROX_MAX_LEN, APPROX_SCRATCH_BYTES, approx_row_bytes, pass) == 1 && pass[0][3] == 400, "few queries");
	CHECK(two > 0, "no case had two launches");
	CHECK(budget_found(-3) == 1 && budget_found(-2) == 0 && budget_found(-1) == 0 && budget_found(0) == 0 && budget_found(1) == 1 && budget_found(INT64_MIN + 2) == INT64_MAX - 3,
	      "what a cnt says was found");
	return n;
}

// the substitutions: push in decreasing position, read back, pop
static long check_packing()
{
	long n = 0;
	for (int t = 0; t < 2000; ++t) {
		const int k = (int)(rnd() % (APPROX_MAX_MM + 1));
		std::vector<int64_t> pos;
		while ((int)pos.size() < k) { const int64_t p = t < 4 ? (int64_t)pos.size() * (t & 1 ? 1 : 2730) + (t & 2 ? 0 : 1) : (int64_t)(rnd() % APPROX_MAX_LEN); if (std::find(pos.begin(), pos.end(), p) == pos.end()) pos.push_back(p); }
		std::sort(pos.rbegin(), pos.rend());
		uint64_t subs = 0, hist[APPROX_MAX_MM + 1] = {0};
		int sym[APPROX_MAX_MM];
		for (int m = 0; m < k; ++m) { sym[m] = 1 + (int)(rnd() % 4); hist[m] = subs; subs = approx_push(subs, m, pos[m], sym[m]); }
		for (int m = 0; m < APPROX_MAX_MM; ++m) {
			const uint64_t f = subs >> (16 * m) & 0xffff;
			CHECK((f != 0) == (m < k), "field %d of %d", m, k);
			if (m < k) CHECK(approx_sub_pos(subs, m) == pos[m] && approx_sub_sym(subs, m) == sym[m] && f == ((uint64_t)pos[m] << 3 | (uint64_t)sym[m]), "field %d", m);
		}
		for (int m = k; m > 0; --m) { subs = approx_pop(subs, m); CHECK(subs == hist[m - 1], "pop %d", m); }
		CHECK(subs == 0, "pop");
		++n;
	}
	CHECK(approx_push(0, 3, APPROX_MAX_LEN - 1, 4) == 0xfffcull << 48 && approx_push(0, 0, 0, 1) == 1, "the largest and the smallest field");
	return n;
}

// the piece bound over tiny sets of strings: the interval of a word is (id * BIG, id * BIG + occurrences), the empty word (0, N)
struct Texts {
	std::vector<std::string> s;                                // symbols as the characters 1 .. 5
	std::map<std::string, int64_t> id;
	std::vector<std::string> word;
	static const int64_t BIG = 1 << 20;
	int64_t N = 0;
	int64_t count(const std::string &w) const
	{
		int64_t c = 0;
		for (const std::string &t : s)
			for (size_t i = 0; i + w.size() <= t.size(); ++i) c += t.compare(i, w.size(), w) == 0;
		return c;
	}
	void reset() { id.clear(); word.clear(); id[""] = 0; word.push_back(""); }
	void step(int64_t lo, int64_t hi, int c, int64_t &nlo, int64_t &nhi)
	{
		const std::string &w = word[(size_t)(lo / BIG)];
		CHECK(hi - lo == (w.empty() ? N : count(w)), "the bound handed back an interval it was not given");
		const std::string nw = std::string(1, (char)c) + w;
		if (!id.count(nw)) { id[nw] = (int64_t)word.size(); word.push_back(nw); }
		nlo = id[nw] * BIG; nhi = nlo + count(nw);
	}
};

static long check_bound()
{
	long n = 0, positive = 0, tight = 0, early = 0, starved = 0;
	for (int set = 0; set < 40; ++set) {
		Texts T;
		const int ns = 1 + (int)(rnd() % 6);
		for (int k = 0; k < ns; ++k) {
			std::string t;
			const int len = (int)(rnd() % 12);
			for (int i = 0; i < len; ++i) t.push_back((char)(set % 3 == 0 ? 1 + rnd() % 2 : rnd() % 10 == 0 ? 5 : 1 + rnd() % 4));
			T.s.push_back(t);
			if (rnd() % 3 == 0) T.s.push_back(t);              // duplicates: min_occ = 2 keeps something
			T.N += (int64_t)t.size() + 1;
		}
		T.N += (int64_t)(T.s.size() - (size_t)ns);
		for (int t = 0; t < 60; ++t) {
			const int L = 1 + (int)(rnd() % 7);
			uint8_t q[8], G[8];
			const std::string &src = T.s[rnd() % T.s.size()];
			for (int i = 0; i < L; ++i) q[i] = (uint8_t)(t % 2 && (size_t)i < src.size() && rnd() % 4 ? src[(size_t)i] : rnd() % 8 == 0 ? 5 : 1 + rnd() % 4);
			for (int64_t min_occ = 1; min_occ <= 2; ++min_occ) {
				// the pieces as the definition states them, one word at a time
				std::vector<std::pair<int, int>> pieces;
				for (int j = L - 1, e = L - 1; j >= 0; --j) {
					std::string w;
					for (int i = j; i <= e; ++i) w.push_back((char)q[i]);
					if (q[j] == 5) { pieces.push_back({j, j}); e = j - 1; }
					else if (T.count(w) < min_occ) { pieces.push_back({j, e}); e = j - 1; }
				}
				int64_t steps = 0;
				T.reset();
				for (int i = 0; i < 8; ++i) G[i] = 0xee;
				const int got = approx_bound(q, L, T.N, min_occ, 8, 1000, [&](int64_t lo, int64_t hi, int c, int64_t &nlo, int64_t &nhi) { T.step(lo, hi, c, nlo, nhi); }, G, &steps);
				CHECK(got == (int)pieces.size(), "set %d: %d pieces, the definition gives %zu", set, got, pieces.size());
				int nn = 0;
				for (int i = 0; i < L; ++i) nn += q[i] == 5;
				CHECK(steps == L - nn, "%lld steps for %d symbols, %d of them N", (long long)steps, L, nn);
				for (int i = L; i < 8; ++i) CHECK(G[i] == 0xee, "G[%d] was written", i);
				for (int p = 0; p < L; ++p) {
					int D = 0;
					for (auto &pc : pieces) D += pc.second <= p;
					CHECK(got - (int)G[p] == D && approx_need(G, got, p + 1) == D, "D[%d] = %d, the definition gives %d", p, got - (int)G[p], D);
					// the fewest substitutions of q[0 .. p] into a word of A C G T with min_occ occurrences: over the windows of the strings
					int best = -1;
					std::map<std::string, int64_t> seen;
					for (const std::string &s : T.s)
						for (size_t i = 0; i + (size_t)p + 1 <= s.size(); ++i) {
							const std::string w = s.substr(i, (size_t)p + 1);
							if (w.find((char)5) != std::string::npos || seen.count(w)) continue;
							seen[w] = 1;
							if (T.count(w) < min_occ) continue;
							int d = 0;
							for (int x = 0; x <= p; ++x) d += w[(size_t)x] != (char)q[x];
							if (best < 0 || d < best) best = d;
						}
					if (best >= 0) { CHECK(D <= best, "set %d min_occ %lld: D[%d] = %d but %d substitutions suffice", set, (long long)min_occ, p, D, best); tight += D == best; positive += D > 0; }
				}
				CHECK(approx_need(G, got, 0) == 0, "D[-1]");
				// the early exits
				for (int mm = 0; mm <= APPROX_MAX_MM; ++mm) {
					int64_t st = 0;
					T.reset();
					const int r = approx_bound(q, L, T.N, min_occ, mm, 1000, [&](int64_t lo, int64_t hi, int c, int64_t &nlo, int64_t &nhi) { T.step(lo, hi, c, nlo, nhi); }, G, &st);
					CHECK(r == std::min(got, mm + 1) && st <= steps, "max_mm %d: %d of %d pieces", mm, r, got);
					early += r < got;
				}
				for (int64_t ms = 0; ms <= L; ++ms) {
					int64_t st = 0;
					T.reset();
					const int r = approx_bound(q, L, T.N, min_occ, 8, ms, [&](int64_t lo, int64_t hi, int c, int64_t &nlo, int64_t &nhi) { T.step(lo, hi, c, nlo, nhi); }, G, &st);
					CHECK(st <= ms && (ms < steps ? r == -1 && st == ms : r == got), "max_steps %lld: %d after %lld steps", (long long)ms, r, (long long)st);
					starved += r == -1;
				}
				++n;
			}
		}
	}
	CHECK(positive > 500 && tight > 2000 && early > 100 && starved > 1000, "weak cases: %ld positive, %ld tight, %ld early, %ld starved", positive, tight, early, starved);
	return n;
}

int main()
{
	const long a = check_launches(), b = check_packing(), c = check_bound();
	printf("APPROX PLAN OK %ld launches %ld packings %ld bounds\n", a, b, c);
	return 0;
}
