// The arithmetic of the k-mer enumeration (rb2_hip_kmers: kernel k_kmer_expand in rb2_query.h, host side in rb2_query_host.h) that needs no
// GPU: the packing of a k-mer, the reverse complement of a packed k-mer, how many items the depth-first walk takes from a frontier
// segment, how large a segment can get, and when the record staging buffer must be emptied.  Plain C++ with no HIP in it, so that a CPU
// program can include it (tests/test_kmer_plan.py); the functions are constexpr, which also makes them callable from the kernel.
#pragma once
#include <cstdint>

/* a k-mer is packed two bits per symbol, A C G T = 0 1 2 3 (nt6 code - 1), the symbol at text position p at bits 2 * (k - 1 - p): the
 * numeric order of the codes of one k is the lexicographic order of the k-mers.  k = 1 .. 32 */
static const int KMER_MAX_K = 32;

/* the code of the k-mer whose FIRST symbol is the nt6 code a (1 .. 4) and whose other l symbols are the l-mer `code`: the backward step */
constexpr uint64_t kmer_prepend(uint64_t code, int l, int a) { return code | (uint64_t)(a - 1) << (2 * l); }

/* the nt6 code (1 .. 4) at text position p of a packed k-mer */
constexpr int kmer_symbol(uint64_t code, int k, int p) { return (int)(code >> (2 * (k - 1 - p)) & 3) + 1; }

/* the 32 two-bit groups of x in reverse order */
constexpr uint64_t kmer_rev2(uint64_t x)
{
	x = (x >> 2 & 0x3333333333333333ull) | (x & 0x3333333333333333ull) << 2;
	x = (x >> 4 & 0x0f0f0f0f0f0f0f0full) | (x & 0x0f0f0f0f0f0f0f0full) << 4;
	x = (x >> 8 & 0x00ff00ff00ff00ffull) | (x & 0x00ff00ff00ff00ffull) << 8;
	x = (x >> 16 & 0x0000ffff0000ffffull) | (x & 0x0000ffff0000ffffull) << 16;
	return x >> 32 | x << 32;
}

/* the code of the reverse complement of a packed k-mer (the complement of a two-bit symbol is its bitwise not: A <-> T, C <-> G) */
constexpr uint64_t kmer_revcomp(uint64_t code, int k) { return ~kmer_rev2(code) >> (64 - 2 * k); }

/* is this k-mer the one of the pair (itself, reverse complement) that a canonical enumeration reports?  A palindrome is its own pair */
constexpr bool kmer_canonical(uint64_t code, int k) { return code <= kmer_revcomp(code, k); }

/* The walk keeps one segment of at most F items per level and expands the top one slice by slice; an item has at most four children, so
 * a slice of F / 4 items never overfills the fresh segment of the next level.  F >= 4. */
static const int64_t KMER_FRONTIER_MIN = 4;

/* items of the next slice of a segment that holds avail (>= 1) of them */
constexpr int64_t kmer_slice(int64_t avail, int64_t F) { return avail < F / 4 ? avail : F / 4; }

/* the most items the segment of level l (l-mers, 0 <= l <= 32) ever holds in an index of N rows: F, the 4^l l-mers there are, and N
 * (distinct l-mers that occur have disjoint non-empty intervals of rows) */
constexpr int64_t kmer_segment_cap(int l, int64_t F, int64_t N)
{
	int64_t c = F < N ? F : N;
	if (l < 31 && ((int64_t)1 << (2 * l)) < c) c = (int64_t)1 << (2 * l);
	return c < 1 ? 1 : c;
}

/* Records: the k-mer that draws number j (0, 1, ...: the device cursor, which ends as the number of k-mers found) is stored when
 * j < max_recs, in slot j - flushed of a staging buffer of `stage` records, flushed = the records already copied to the caller (always a
 * prefix of the numbers: 0 .. flushed - 1).  stage = min(max_recs, limit), limit >= 4 (one item's children): with room for max_recs
 * nothing is flushed before the end. */
constexpr int64_t kmer_stage_recs(int64_t max_recs, int64_t limit) { return max_recs < limit ? max_recs : limit; }

/* items of the next slice at the last level, whose children are records: no more than the staging buffer holds when it is empty (a
 * buffer that holds all max_recs records never limits the slice: what draws a number beyond them is not stored) */
constexpr int64_t kmer_final_slice(int64_t avail, int64_t F, int64_t stage, int64_t max_recs)
{
	int64_t t = kmer_slice(avail, F);
	if (stage < max_recs && stage / 4 < t) t = stage / 4 < 1 ? 1 : stage / 4;
	return t;
}

/* must the staging buffer be copied out before a slice of `take` items (at most 4 * take records) is expanded, `found` numbers being
 * drawn so far?  The numbers that can still be stored are min(found, max_recs) .. min(found + 4 * take, max_recs) - 1 */
constexpr bool kmer_must_flush(int64_t found, int64_t flushed, int64_t take, int64_t stage, int64_t max_recs)
{
	const int64_t last = found + 4 * take < max_recs ? found + 4 * take : max_recs;
	return last - flushed > stage;
}

/* records the staging buffer holds when `found` numbers are drawn: what a flush copies to the caller's rec + 3 * flushed */
constexpr int64_t kmer_staged(int64_t found, int64_t flushed, int64_t max_recs) { return (found < max_recs ? found : max_recs) - flushed; }
