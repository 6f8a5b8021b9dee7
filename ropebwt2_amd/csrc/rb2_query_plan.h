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

/* ---- approximate search (rb2_hip_approx: kernel k_approx in rb2_query.h, host side in rb2_query_host.h) ----
 * What follows is also compiled into the kernel: the functions are constexpr, or marked for both sides when a HIP compiler reads them. */
#ifdef __HIPCC__
#define RB2_PLAN_HD __host__ __device__
#else
#define RB2_PLAN_HD
#endif

static const int APPROX_MAX_MM = 4;                            /* substitutions of a match at the most: four 16-bit fields of subs */
static const int64_t APPROX_MAX_LEN = 8192;                    /* symbols of a query at the most: a position has 13 bits of a field */
static const int64_t APPROX_ROWS = 16 * 2048;                  /* DPP rows of a launch at the most (2048 blocks: eight per CU); a row takes queries a launch apart */
static const int64_t APPROX_SCRATCH_BYTES = (int64_t)256 << 20;   /* the stacks of all rows of a launch stay under this */
static const int64_t APPROX_SHORT_ROWS = 16 * 1024;            /* rows of the launch that takes the short queries when the lengths are mixed or unknown */

/* subs: the substitutions of a match, 16 bits each as pos << 3 | sym, in the order a backward search meets them (decreasing pos), the
 * first in bits 0 .. 15; sym >= 1, so a used field is never 0 */
constexpr uint64_t approx_push(uint64_t subs, int m, int64_t pos, int sym) { return subs | ((uint64_t)pos << 3 | (uint64_t)sym) << (16 * m); }   /* field m (m fields used) */
constexpr uint64_t approx_pop(uint64_t subs, int m) { return subs & ~(0xffffull << (16 * (m - 1))); }                                               /* drops field m - 1 */
constexpr int64_t approx_sub_pos(uint64_t subs, int k) { return (int64_t)(subs >> (16 * k) & 0xffff) >> 3; }
constexpr int approx_sub_sym(uint64_t subs, int k) { return (int)(subs >> (16 * k) & 7); }

/* the stack of one row for queries of up to L (>= 1) symbols: per position the intervals of the four children (64 bytes), then two
 * bytes per position -- the piece count G of approx_bound, and the child taken with the next one to try -- each array padded to 8 bytes */
constexpr int64_t approx_pad(int64_t L) { return (L + 7) & ~(int64_t)7; }
constexpr int64_t approx_row_bytes(int64_t L) { return 64 * L + 2 * approx_pad(L); }

/* ---- the row stacks of the searches with a step budget (k_approx, k_approx_ed, k_irreducible; DESIGN.md section 16, "the path stack") ----
 * Each family has a row layout of its own (approx_row_bytes, edit_row_bytes in rb2_edit_plan.h, irred_row_bytes); what follows takes it as
 * row_bytes, or as row_bytes_of(L) for the two whose rows are sized by the length of a query: at least 64 L bytes, non-decreasing in L. */

/* what an item has found, from its cnt as these searches (and rb2_hip_correct) report it: >= 0 found, -1 malformed, <= -2 out of steps
 * with -2 - cnt found by then */
constexpr int64_t budget_found(int64_t c) { return c >= 0 ? c : c <= -2 ? -2 - c : 0; }

/* rows of a launch over n (>= 1) queries with stacks of row_bytes each in `bytes` of scratch: at most n and max_rows, one at the least */
constexpr int64_t stack_rows(int64_t n, int64_t row_bytes, int64_t bytes, int64_t max_rows)
{
	int64_t r = bytes / row_bytes;
	if (r > max_rows) r = max_rows;
	if (r > n) r = n;
	return r < 1 ? 1 : r;
}

/* the longest query the stacks of `rows` rows hold in `bytes` of scratch (0: none), APPROX_MAX_LEN at the most */
template <typename RB> constexpr int64_t stack_len_cap(int64_t rows, int64_t bytes, RB row_bytes_of)
{
	int64_t L = bytes / rows / 64;                             /* no longer one fits: a row is at least 64 L bytes */
	if (L > APPROX_MAX_LEN) L = APPROX_MAX_LEN;
	while (L > 0 && row_bytes_of(L) * rows > bytes) --L;
	return L;
}

/* A call is one launch when every query is short enough for APPROX_SHORT_ROWS rows (or there are no more queries than rows anyway);
 * else two: the first takes the queries of up to `cut` symbols on many rows, the second the longer ones on the rows that lmax allows.
 * lmax = the longest query (APPROX_MAX_LEN when the lengths are not known to the host, as in the _dev variants), at least 1.
 * pass[k] = {lmin, lcap, lrow, rows}: the launch takes the queries with lmin < length <= lcap on `rows` rows with stacks for lrow symbols;
 * returns the number of launches.  Every length, negative and oversized ones included, belongs to exactly one launch. */
template <typename RB> static inline int stack_passes(int64_t n, int64_t lmax, int64_t bytes, RB row_bytes_of, int64_t pass[2][4])
{
	const int64_t all = stack_rows(n, row_bytes_of(lmax), bytes, APPROX_ROWS), cut = stack_len_cap(APPROX_SHORT_ROWS, bytes, row_bytes_of);
	if (all >= n || all >= APPROX_SHORT_ROWS || lmax <= cut || cut < 1) {
		pass[0][0] = INT64_MIN; pass[0][1] = INT64_MAX; pass[0][2] = lmax; pass[0][3] = all;
		return 1;
	}
	pass[0][0] = INT64_MIN; pass[0][1] = cut; pass[0][2] = cut; pass[0][3] = stack_rows(n, row_bytes_of(cut), bytes, APPROX_ROWS);
	pass[1][0] = cut; pass[1][1] = INT64_MAX; pass[1][2] = lmax; pass[1][3] = all;
	return 2;
}

/* The piece bound.  One backward search over q[0 .. L) (nt6 codes 1 .. 5) from its last symbol: when the interval of q[s .. e] holds
 * fewer than min_occ rows, [s, e] is a piece and the search starts again at s - 1 from the whole index [0, N); an N (5) is a piece by
 * itself (the symbols behind it that still matched are no piece).  No string with min_occ occurrences contains a piece unchanged and the
 * pieces are disjoint, so a match of q needs at least D[p] = (pieces that lie wholly in [0, p]) substitutions in q[0 .. p].
 * step(lo, hi, c, nlo, nhi) must set [nlo, nhi) to the interval of c followed by the word of [lo, hi): one pair of ranks, counted in *steps.
 * G[p] = the pieces whose last position lies behind p, so that D[p] = pieces - G[p].  Returns the number of pieces; stops early with
 * max_mm + 1 once there are more than max_mm (G is then incomplete: no match exists), and with -1 when *steps reached max_steps. */
template <typename F>
RB2_PLAN_HD inline int approx_bound(const uint8_t *q, int64_t L, int64_t N, int64_t min_occ, int max_mm, int64_t max_steps, F step, uint8_t *G, int64_t *steps)
{
	int pieces = 0;
	int64_t lo = 0, hi = N, e = L - 1;                         /* the interval of q[j + 1 .. e]: the run that may become a piece */
	for (int64_t j = L - 1; j >= 0; --j) {
		const int c = q[j];
		bool cut = c == 5, piece = false;
		if (!cut) {
			if (*steps >= max_steps) return -1;
			++*steps;
			int64_t nlo = 0, nhi = 0;
			step(lo, hi, c, nlo, nhi);
			if (nhi - nlo < min_occ) cut = piece = true;
			else { lo = nlo; hi = nhi; }
		}
		if (!cut && j > 0) continue;
		/* the run ends here, as the piece [j, e], in front of an N, or at the first symbol: only now is G known for its positions.
		 * The pieces found so far all end behind e; the piece [j, e] itself ends behind every position of the run but e */
		for (int64_t x = j; x <= e; ++x) G[x] = (uint8_t)(pieces + (piece && x < e));
		if (cut) {
			if (++pieces > max_mm) return pieces;
			lo = 0; hi = N; e = j - 1;
		}
	}
	return pieces;
}

/* D[p - 1] from what approx_bound left: the substitutions every match needs in front of position p */
RB2_PLAN_HD inline int approx_need(const uint8_t *G, int pieces, int64_t p) { return p > 0 ? pieces - (int)G[p - 1] : 0; }

/* ---- irreducible overlaps (rb2_hip_irreducible: kernel k_irreducible in rb2_query.h, host side in rb2_query_host.h) ----
 * The stack of a row is a list of entries, the frames of the nodes on the current path behind each other (frame d = the entries of the
 * node at depth d, in increasing overlap length).  An entry is written when it is ranked, and every pair of ranks is a step. */
static const int64_t IRRED_MAX_LEN = 8192;                     /* symbols of a query, and of an extension, at the most: an overlap length has 16 bits */
static const int64_t IRRED_ROWS = 16 * 2048;                   /* DPP rows of a launch at the most (2048 blocks: eight per CU); a row takes queries a launch apart */
static const int64_t IRRED_SCRATCH_BYTES = (int64_t)256 << 20; /* the stacks of all rows of a launch stay under this (one row may be larger alone) */

/* entries a row holds at the most for queries of up to lmax symbols (1 .. IRRED_MAX_LEN), min_ovlp >= 1, max_ext in 1 .. IRRED_MAX_LEN and
 * max_steps >= 1: the frames 0 .. max_ext of a path hold at most lmax - min_ovlp entries each (the overlap lengths min_ovlp .. lmax - 1),
 * and no more entries are ever written than steps taken; one at the least */
constexpr int64_t irred_entry_cap(int64_t lmax, int64_t min_ovlp, int64_t max_ext, int64_t max_steps)
{
	int64_t e = lmax > min_ovlp ? (lmax - min_ovlp) * (max_ext + 1) : 0;
	if (e > max_steps) e = max_steps;
	return e < 1 ? 1 : e;
}

/* frames whose first entry and next child a row remembers: a frame below the top one was pushed at a depth below max_ext, and every frame
 * of the path holds at least one of the cap entries */
constexpr int64_t irred_frames(int64_t cap, int64_t max_ext) { return cap < max_ext ? cap : max_ext; }

constexpr int64_t irred_pad(int64_t bytes) { return (bytes + 7) & ~(int64_t)7; }

/* the stack of one row: per entry the intervals of its four children (64 bytes: one line) and its overlap length (2 bytes), per frame
 * its first entry (4 bytes) and the next child to try (1 byte), each array padded to 8 bytes */
constexpr int64_t irred_row_bytes(int64_t cap, int64_t max_ext)
{
	return 64 * cap + irred_pad(4 * irred_frames(cap, max_ext)) + irred_pad(2 * cap) + irred_pad(irred_frames(cap, max_ext));
}
