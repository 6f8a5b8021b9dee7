// The arithmetic of the .fmd encoder (rb2_hip_save_fmd: kernels in rb2_fmd_save.h) that needs no GPU: the code of a run,
// the header of a block, how many payload bits a block has, where the block that starts at a run ends (a bisection over the prefix sum of the
// code widths), the rank-frame rule, and the packing of the small records the kernels hand to each other.  Plain C++, marked for both sides
// when a HIP compiler reads it, so that a CPU program can include it (tests/test_fmd_plan.py checks a serial encoder made of these functions
// alone against the host writer, csrc/host/fmd.c, which restates rld0.c).
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define RB2_FMDS_HD __host__ __device__ __forceinline__
#else
#define RB2_FMDS_HD inline
#endif

static const uint32_t FMDS_BW = 8;                 /* words per block */
static const uint32_t FMDS_CHUNK_BLOCKS = 1u << 20;   /* blocks per chunk of 2^23 words: the last one of a chunk gives up one payload word */
static const uint32_t FMDS_MAX_RUNS = 96;          /* a block holds fewer runs than this: 384 payload bits, 4 bits for the shortest code */
static const uint32_t FMDS_SEG_MIN = 96;           /* runs per segment at the least: a block that starts in one segment ends in it or in the next */

RB2_FMDS_HD int fmds_ilog2(uint64_t v)             /* ilog2(0) = -1 (rld0.c:26-43) */
{
	int r = -1;
	if (v >> 32) { r += 32; v >>= 32; }
	if (v >> 16) { r += 16; v >>= 16; }
	if (v >> 8) { r += 8; v >>= 8; }
	if (v >> 4) { r += 4; v >>= 4; }
	if (v >> 2) { r += 2; v >>= 2; }
	if (v >> 1) { r += 1; v >>= 1; }
	return r + (int)v;
}

/* a run of l symbols c (1 <= l < 2^51): Elias delta of l, then three bits of c, w <= 64 bits, placed most significant bit first */
RB2_FMDS_HD uint32_t fmds_width(uint64_t l)
{
	const int y = fmds_ilog2(l), z = fmds_ilog2((uint64_t)y + 1);
	return (uint32_t)(2 * z + 1 + y + 3);
}
RB2_FMDS_HD uint64_t fmds_code(uint64_t l, uint32_t c)
{
	const int y = fmds_ilog2(l);
	return (((l ^ (1ull << y)) | (uint64_t)(y + 1) << y) << 3) | (uint64_t)c;
}

/* the header of a block holds the symbols of the PREVIOUS block: its total T chooses the width of the seven fields */
RB2_FMDS_HD uint32_t fmds_type(uint64_t T) { return T < 0x4000ull ? 0u : T < 0x40000000ull ? 1u : 2u; }
RB2_FMDS_HD uint32_t fmds_hdr_words(uint32_t type) { return type == 0 ? 2u : type == 1 ? 4u : 7u; }
/* word i (i < 7) of the header of type `type` for the counts cnt[0] = T, cnt[1..6] = the six symbols */
RB2_FMDS_HD uint64_t fmds_hdr_word(uint32_t type, const uint64_t cnt[7], uint32_t i)
{
	uint64_t v = 0;
	if (type == 0) { if (i < 2) for (uint32_t k = 0; k < 4 && 4 * i + k < 7; ++k) v |= (cnt[4 * i + k] & 0xffffull) << (16 * k); }
	else if (type == 1) { if (i < 4) for (uint32_t k = 0; k < 2 && 2 * i + k < 7; ++k) v |= (cnt[2 * i + k] & 0xffffffffull) << (32 * k); }
	else v = cnt[i];
	if (i == 0) v |= (uint64_t)type << 62;
	return v;
}

/* block number blk (its header is word 8 * blk of the stream) is the last of its chunk */
RB2_FMDS_HD bool fmds_chunk_last(uint64_t blk) { return (blk + 1) % FMDS_CHUNK_BLOCKS == 0; }
/* payload bits of a block: the words behind its header up to word 7, or word 6 in the last block of a chunk */
RB2_FMDS_HD uint32_t fmds_payload_bits(uint32_t type, bool chunk_last) { return (FMDS_BW - fmds_hdr_words(type) - (chunk_last ? 1u : 0u)) * 64u; }

/* THE FIT RULE.  With u payload bits of a block of C used, a code of w bits does not fit iff u + w >= C and u > C - 64: the writer asks
 * `w >= free bits of the word && the cursor stands in the last word`, and its cursor moves on only when a code spills, so from u == C - 64
 * any code fits (a 64-bit one fills the block to its last bit), while a code never fills the last bit from inside the last word.  The first code
 * of a block is placed without the question being asked again, which u > C - 64 says too (C >= 64).  u + w is monotone along the runs, so the
 * block that starts at run i ends at the first j with W[j + 1] - W[i] >= C (W: prefix sum of the widths, W[0 .. n] for n runs), corrected by
 * one run when the exception applies.  Returns the first run of the next block; *complete = false (and n) when the n runs do not fill the block.
 * (A 64-bit code -- a run of 2^50 symbols or more -- that arrives right behind a code that ended on a word boundary makes the writer, like
 * rld0.c:145, shift a word by 64; what the format is there nobody can say.  These functions place it like any other code.) */
template <typename WT> RB2_FMDS_HD uint64_t fmds_block_end(const WT *W, uint64_t i, uint64_t n, uint32_t C, bool *complete)
{
	const uint64_t w0 = (uint64_t)W[i];
	uint64_t lo = i, hi = i + FMDS_MAX_RUNS + 1 < n ? i + FMDS_MAX_RUNS + 1 : n;   /* the answer, if any, is in [i, hi) */
	if (lo >= hi || (uint64_t)W[hi] - w0 < C) { *complete = false; return n; }
	while (lo + 1 < hi) {                                      /* invariant: W[hi] - w0 >= C; the smallest j with W[j + 1] - w0 >= C is in [lo, hi) */
		const uint64_t mid = (lo + hi) >> 1;
		if ((uint64_t)W[mid] - w0 >= C) hi = mid; else lo = mid;
	}
	*complete = true;
	const uint64_t u = (uint64_t)W[lo] - w0;
	return u + 64 > C ? lo : lo + 1;
}

/* where a code of w bits goes when u payload bits are used: payload word wi gets hi ORed in, and word wi + 1 gets lo when spill is set */
struct FmdsPlace { uint32_t wi; bool spill; uint64_t hi, lo; };
RB2_FMDS_HD FmdsPlace fmds_place(uint32_t u, uint64_t x, uint32_t w)
{
	FmdsPlace p;
	const uint32_t o = u & 63u;
	p.wi = u >> 6; p.lo = 0;
	p.spill = o + w > 64;
	if (!p.spill) p.hi = x << (64 - o - w);
	else { const uint32_t s = o + w - 64; p.hi = x >> s; p.lo = x << (64 - s); }
	return p;
}

/* THE FRAME RULE (fmd_index_mt): the stream of n_bytes has n_blks blocks, a frame covers 2^ibits symbols, and frame k >= 1 describes the
 * LAST header whose cumulative symbol count S has (S >> ibits) + 1 == k */
RB2_FMDS_HD int fmds_ibits(uint64_t total, uint64_t n_bytes) { return fmds_ilog2(total / (n_bytes / 64 + 1)) + 4; }
RB2_FMDS_HD uint64_t fmds_n_frames(uint64_t total, int ibits) { return ((total + (1ull << ibits) - 1) >> ibits) + 1; }
RB2_FMDS_HD uint64_t fmds_frame_of(uint64_t S, int ibits) { return (S >> ibits) + 1; }
RB2_FMDS_HD uint64_t fmds_image_size(uint64_t n_bytes, uint64_t n_frames) { return 80 + n_bytes + 56 * n_frames; }

/* The encoder keeps, per bucket of 2^bbits symbols, the last header whose S falls into it; frames of 2^ibits symbols are read off that table
 * when the stream is complete (ibits depends on its length), which needs ibits >= bbits.  bbits is the smallest that keeps the table within
 * cap entries. */
RB2_FMDS_HD int fmds_bucket_bits(uint64_t total, uint64_t cap) { int b = 0; while ((total >> b) + 2 > cap) ++b; return b; }
/* the last bucket of frame k (k >= 1), clamped to the nb buckets of the table */
RB2_FMDS_HD uint64_t fmds_frame_last_bucket(uint64_t k, int ibits, int bbits, uint64_t nb)
{
	const int d = ibits - bbits;
	if (d >= 63 || (k << d) >> d != k || (k << d) - 1 >= nb) return nb - 1;
	return (k << d) - 1;
}

/* next[i] of run i: for each header type t of a block that starts at run i, in bits [9t, 9t + 9): the number of runs the block holds (7 bits;
 * FMDS_STOP: the runs known so far do not fill it, FMDS_FINAL: i is behind the last run -- the block is the closing header) and the type of the block behind it */
static const uint32_t FMDS_STOP = 127, FMDS_FINAL = 126;
RB2_FMDS_HD uint32_t fmds_next_pack(uint32_t t, uint32_t delta, uint32_t type2) { return (delta | type2 << 7) << (9 * t); }
RB2_FMDS_HD uint32_t fmds_next_delta(uint32_t v, uint32_t t) { return (v >> (9 * t)) & 127u; }
RB2_FMDS_HD uint32_t fmds_next_type(uint32_t v, uint32_t t) { return (v >> (9 * t + 7)) & 3u; }

/* Where a walk along next[] that enters a segment (or a group of segments) in state (run, type) leaves it, and how many blocks it opened on the way:
 * `run` counts from the first run of the NEXT segment (< 96), or from the first run of the batch when the walk stopped (stop = 1: at a block the known
 * runs do not fill, which is not counted; stop = 2: behind the closing header, which is). */
RB2_FMDS_HD uint64_t fmds_exit_pack(uint64_t run, uint32_t type, uint32_t stop, uint64_t nblk) { return run | (uint64_t)type << 28 | (uint64_t)stop << 30 | nblk << 32; }
RB2_FMDS_HD uint64_t fmds_exit_run(uint64_t e) { return e & 0xfffffffull; }
RB2_FMDS_HD uint32_t fmds_exit_type(uint64_t e) { return (uint32_t)(e >> 28) & 3u; }
RB2_FMDS_HD uint32_t fmds_exit_stop(uint64_t e) { return (uint32_t)(e >> 30) & 3u; }
RB2_FMDS_HD uint64_t fmds_exit_nblk(uint64_t e) { return e >> 32; }
static const uint32_t FMDS_ENTRIES = FMDS_MAX_RUNS * 3;    /* entry states of a segment: (run < 96, type) */
