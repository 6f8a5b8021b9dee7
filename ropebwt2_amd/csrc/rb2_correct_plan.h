// Correcting a read by the k-mer spectrum of the index (rb2_hip_correct: kernel k_correct in rb2_correct.h, host side in
// rb2_query_host.h): the rule itself and the launch arithmetic, plain C++ with no HIP in it.  The kernel and
// tests/correct_plan_check.cpp compile the same text (correct_read is marked for both sides when a HIP compiler reads it).
#pragma once
#include <cstdint>
#include "rb2_query_plan.h"

static const int64_t CORRECT_MAX_LEN = 8192;                   /* symbols of a read at the most: its solid bits are 1 KiB of LDS */
static const int64_t CORRECT_ROWS = 16 * 2048;                 /* DPP rows of a launch at the most (2048 blocks: eight per CU); a row takes reads a launch apart */

/* the solid bits of a read of L symbols: one bit per window, L windows at the most (k = 1), in 32-bit words */
constexpr int64_t correct_solid_words(int64_t L) { return (L + 31) / 32; }
static const int CORRECT_SOLID_WORDS = (int)correct_solid_words(CORRECT_MAX_LEN);
constexpr int64_t correct_solid_bytes(int64_t rows) { return rows * 4 * correct_solid_words(CORRECT_MAX_LEN); }

/* rows of a launch over n (>= 1) reads when no more than cap (>= 1) are wanted: at most n, cap and CORRECT_ROWS, one at the least */
constexpr int64_t correct_rows(int64_t n, int64_t cap)
{
	int64_t r = cap < CORRECT_ROWS ? cap : CORRECT_ROWS;
	if (r > n) r = n;
	return r < 1 ? 1 : r;
}

/* what HipBwt.correct takes for max_probes when the caller names none: the profile of a read of L symbols (L - k + 1 <= L probes) and
 * `attempts` tried windows behind it, each three alternatives and, for one that fixes, the k windows around the fix at the most */
constexpr int64_t correct_default_probes(int64_t L, int64_t k, int64_t attempts) { return L + attempts * (3 + k); }

constexpr bool correct_acgt(int c) { return c >= 1 && c <= 4; }

/* cnt and weak of a read as include/rb2_hip.h states them */
struct CorrectOut { int64_t cnt, weak; };

/* The windows j0 .. j1 of the read, in increasing j: a clean one is probed (one probe each, counted against max_probes), the others are
 * not solid.  false: the budget ran out before a probe (the bits from that window on are as they were). */
template <typename Q, typename S, typename P>
RB2_PLAN_HD inline bool correct_eval(Q &q, S &solid, int64_t k, int64_t min_occ, int64_t max_probes, int64_t j0, int64_t j1, int64_t &probes, P &probe)
{
	int64_t lastbad = j0 - 1;                                  /* the last position in front of the window's end that is no A C G T */
	for (int64_t x = j0; x < j0 + k - 1; ++x) if (!correct_acgt(q.get(x))) lastbad = x;
	for (int64_t j = j0; j <= j1; ++j) {
		if (!correct_acgt(q.get(j + k - 1))) lastbad = j + k - 1;
		if (lastbad >= j) { solid.set(j, false); continue; }
		if (probes >= max_probes) return false;
		++probes;
		solid.set(j, probe(j, (int64_t)-1, 0) >= min_occ);
	}
	return true;
}

/* The rule (include/rb2_hip.h, "correcting reads").  q.get(x) = symbol x of the read (nt6 codes 1 .. 5), q.set(p, b) changes it;
 * solid.get(j) / solid.set(j, v) = the bit of window j; probe(j, p, b) = the occurrences of window j with b at position p (p < 0: as
 * it stands), called for clean words only.  L <= CORRECT_MAX_LEN, k, min_occ, max_fix, max_probes >= 1.
 * Position p is weak when no solid window contains it: going through p = 0, 1, ... with `last` = the largest solid window <= min(p, L - k),
 * that is last < p - k + 1. */
template <typename Q, typename S, typename P>
RB2_PLAN_HD inline CorrectOut correct_read(Q &q, S &solid, int64_t L, int64_t k, int64_t min_occ, int64_t max_fix, int64_t max_probes, P probe, int64_t *probes_out = nullptr)
{
	int64_t probes = 0, fixes = 0;
	if (probes_out) *probes_out = 0;
	if (L < k) return {0, L};
	const int64_t nw = L - k + 1;
	bool over = !correct_eval(q, solid, k, min_occ, max_probes, 0, nw - 1, probes, probe);
	while (!over && fixes < max_fix) {
		bool fixed = false;
		int64_t last = -1;
		for (int64_t p = 0; p < L && !fixed && !over; ++p) {
			if (p < nw && solid.get(p)) last = p;
			if (last >= 0 && last >= p - k + 1) continue;          /* a solid window holds p */
			const int64_t ja = p >= k - 1 ? p - k + 1 : 0, jb = p + k <= L ? p : L - k;
			const int c = q.get(p);
			for (int t = 0; t < 2 && !fixed && !over; ++t) {
				const int64_t j = t ? jb : ja;
				if (t && jb == ja) break;
				bool clean = true;
				for (int64_t x = j; x < j + k && clean; ++x) clean = x == p || correct_acgt(q.get(x));
				if (!clean) continue;
				int ns = 0, bs = 0;
				for (int b = 1; b <= 4 && !over; ++b) {
					if (b == c) continue;
					if (probes >= max_probes) { over = true; break; }
					++probes;
					if (probe(j, p, b) >= min_occ) { ++ns; bs = b; }
				}
				if (over || ns != 1) continue;
				q.set(p, bs);
				++fixes;
				fixed = true;
				over = !correct_eval(q, solid, k, min_occ, max_probes, p >= k - 1 ? p - k + 1 : 0, p < nw ? p : nw - 1, probes, probe);
			}
		}
		if (!fixed) break;
	}
	if (probes_out) *probes_out = probes;
	if (over) return {-2 - fixes, -1};
	int64_t weak = 0, last = -1;
	for (int64_t p = 0; p < L; ++p) {
		if (p < nw && solid.get(p)) last = p;
		weak += !(last >= 0 && last >= p - k + 1);
	}
	return {fixes, weak};
}
