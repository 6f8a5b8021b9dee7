// Stand-alone check of csrc/rb2_correct_plan.h (tests/test_correct_plan.py builds and runs it, once plain and once under ASan + UBSan):
// correct_read, the text the kernel compiles, against a brute force over tiny string sets -- counts by sliding windows, the rule restated
// naively with every window counted again and the weak set recomputed after every fix -- for every k from 1 to L + 1, min_occ 1 .. 3,
// max_fix 1 and 8 and every budget from 1 to one above what the read needs; and the launch arithmetic.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "rb2_correct_plan.h"

typedef std::vector<uint8_t> Str;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng_state >> 33) % n; }

static int64_t occ(const std::vector<Str> &set, const Str &w)
{
	int64_t n = 0;
	for (const Str &s : set)
		for (size_t i = 0; i + w.size() <= s.size(); ++i) {
			bool eq = true;
			for (size_t x = 0; x < w.size() && eq; ++x) eq = s[i + x] == w[x];
			n += eq;
		}
	return n;
}

struct Res { Str text; int64_t cnt, weak, probes; };
static bool same(const Res &a, const Res &b) { return a.text == b.text && a.cnt == b.cnt && a.weak == b.weak && a.probes == b.probes; }

struct VecQ { Str &v; int get(int64_t x) const { return v.at((size_t)x); } void set(int64_t p, int b) { v.at((size_t)p) = (uint8_t)b; } };
struct VecS {
	std::vector<uint32_t> &w;
	bool get(int64_t j) const { return w.at((size_t)(j >> 5)) >> (j & 31) & 1; }
	void set(int64_t j, bool v) { uint32_t &x = w.at((size_t)(j >> 5)); x = v ? x | 1u << (j & 31) : x & ~(1u << (j & 31)); }
};

static Res by_plan(const std::vector<Str> &set, const Str &q, int64_t k, int64_t min_occ, int64_t max_fix, int64_t max_probes)
{
	Res r = {q, 0, 0, 0};
	std::vector<uint32_t> bits((size_t)correct_solid_words((int64_t)q.size()), 0xffffffffu);   // (whatever stood there before)
	VecQ Q = {r.text}; VecS S = {bits};
	const CorrectOut o = correct_read(Q, S, (int64_t)q.size(), k, min_occ, max_fix, max_probes, [&](int64_t j, int64_t p, int b) {
		Str w(r.text.begin() + j, r.text.begin() + j + k);
		if (p >= 0) w.at((size_t)(p - j)) = (uint8_t)b;
		for (uint8_t c : w) if (!correct_acgt(c)) { printf("a probe of a word that is not clean\n"); exit(1); }
		return occ(set, w); }, &r.probes);
	r.cnt = o.cnt; r.weak = o.weak;
	return r;
}

static Res naive(const std::vector<Str> &set, const Str &q0, int64_t k, int64_t min_occ, int64_t max_fix, int64_t max_probes)
{
	Str q = q0;
	const int64_t L = (int64_t)q.size();
	if (L < k) return {q, 0, L, 0};
	auto clean = [&](int64_t j, int64_t but) { for (int64_t x = j; x < j + k; ++x) if (x != but && !correct_acgt(q[(size_t)x])) return false; return true; };
	auto weak = [&]() {
		std::vector<int64_t> w;
		for (int64_t p = 0; p < L; ++p) {
			bool held = false;
			for (int64_t j = 0; j + k <= L; ++j)
				if (j <= p && p < j + k && clean(j, -1) && occ(set, Str(q.begin() + j, q.begin() + j + k)) >= min_occ) held = true;
			if (!held) w.push_back(p);
		}
		return w; };
	int64_t probes = 0, fixes = 0;
	for (int64_t j = 0; j + k <= L; ++j) probes += clean(j, -1);
	if (probes > max_probes) return {q, -2, -1, max_probes};
	while (fixes < max_fix) {
		bool fixed = false;
		for (int64_t p : weak()) {
			const int64_t cand[2] = {p - k + 1 > 0 ? p - k + 1 : 0, p < L - k ? p : L - k};
			for (int t = 0; t < 2 && !fixed; ++t) {
				const int64_t j = cand[t];
				if ((t && j == cand[0]) || !clean(j, p)) continue;
				int ns = 0, bs = 0, alts = 0;
				for (int b = 1; b <= 4; ++b) {
					if (b == q[(size_t)p]) continue;
					++alts;
					Str w(q.begin() + j, q.begin() + j + k);
					w[(size_t)(p - j)] = (uint8_t)b;
					if (occ(set, w) >= min_occ) { ++ns; bs = b; }
				}
				if (probes + alts > max_probes) return {q, -2 - fixes, -1, max_probes};
				probes += alts;
				if (ns != 1) continue;
				q[(size_t)p] = (uint8_t)bs; ++fixes; fixed = true;
				for (int64_t w = 0; w + k <= L; ++w) probes += w <= p && p < w + k && clean(w, -1);
				if (probes > max_probes) return {q, -2 - fixes, -1, max_probes};
			}
			if (fixed) break;
		}
		if (!fixed) break;
	}
	return {q, fixes, (int64_t)weak().size(), probes};
}

int main()
{
	long reads = 0, runs = 0, budgets = 0, fixed = 0, overs = 0, rows = 0;
	for (int round = 0; round < 40; ++round) {
		const uint32_t alpha = 2 + rnd(3);                          // symbols 1 .. alpha, so that words repeat
		std::vector<Str> set(3 + rnd(5));
		for (Str &s : set) { s.resize(rnd(13)); for (uint8_t &c : s) c = rnd(12) ? (uint8_t)(1 + rnd(alpha)) : 5; }
		for (int rd = 0; rd < 6; ++rd) {
			Str q = set[rnd((uint32_t)set.size())];
			if (rd == 5) { q.resize(rnd(10)); for (uint8_t &c : q) c = (uint8_t)(1 + rnd(5)); }
			for (uint32_t m = rnd(3); m > 0 && !q.empty(); --m) q[rnd((uint32_t)q.size())] = rnd(4) ? (uint8_t)(1 + rnd(4)) : 5;
			++reads;
			const int64_t L = (int64_t)q.size();
			for (int64_t k = 1; k <= L + 1; ++k)
				for (int64_t min_occ = 1; min_occ <= 3; ++min_occ)
					for (int64_t max_fix = 1; max_fix <= 8; max_fix += 7) {
						const Res a = by_plan(set, q, k, min_occ, max_fix, (int64_t)1 << 40), b = naive(set, q, k, min_occ, max_fix, (int64_t)1 << 40);
						++runs;
						if (!same(a, b) || a.cnt < 0) { printf("MISMATCH round %d read %d k %lld min_occ %lld max_fix %lld: cnt %lld %lld weak %lld %lld probes %lld %lld\n", round, rd,
							(long long)k, (long long)min_occ, (long long)max_fix, (long long)a.cnt, (long long)b.cnt, (long long)a.weak, (long long)b.weak, (long long)a.probes, (long long)b.probes); return 1; }
						fixed += a.cnt > 0;
						if (L < k && (a.cnt != 0 || a.weak != L || a.text != q)) { printf("a read shorter than k\n"); return 1; }
						for (int64_t mp = 1; mp <= a.probes + 1; ++mp) {    // every budget: it ends in the profile, in the alternatives, in a re-evaluation, or not at all
							const Res c = by_plan(set, q, k, min_occ, max_fix, mp), d = naive(set, q, k, min_occ, max_fix, mp);
							++budgets;
							if (!same(c, d)) { printf("MISMATCH under budget %lld: round %d read %d k %lld min_occ %lld max_fix %lld: cnt %lld %lld\n", (long long)mp, round, rd,
								(long long)k, (long long)min_occ, (long long)max_fix, (long long)c.cnt, (long long)d.cnt); return 1; }
							if ((c.cnt <= -2) != (mp < a.probes) || (mp >= a.probes && !same(c, a))) { printf("budget %lld of %lld probes: cnt %lld\n", (long long)mp, (long long)a.probes, (long long)c.cnt); return 1; }
							overs += c.cnt <= -2;
						}
					}
		}
	}
	// the launch arithmetic
	for (int64_t n = 1; n < 100000; n = n * 3 + 1)
		for (int64_t cap = 1; cap < 100000; cap = cap * 5 + 3) {
			const int64_t r = correct_rows(n, cap);
			++rows;
			if (r < 1 || r > n || r > cap || r > CORRECT_ROWS || (r < n && r < cap && r < CORRECT_ROWS)) { printf("correct_rows(%lld, %lld) = %lld\n", (long long)n, (long long)cap, (long long)r); return 1; }
		}
	if (correct_solid_words(1) != 1 || correct_solid_words(32) != 1 || correct_solid_words(33) != 2 || CORRECT_SOLID_WORDS != 256 || correct_solid_bytes(16) != 16384) { printf("solid words\n"); return 1; }
	if (correct_default_probes(101, 21, 32) != 101 + 32 * 24) { printf("default probes\n"); return 1; }
	printf("CORRECT PLAN OK reads %ld runs %ld budgets %ld fixed %ld over %ld rows %ld\n", reads, runs, budgets, fixed, overs, rows);
	return 0;
}
