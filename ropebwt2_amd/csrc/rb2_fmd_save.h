// The .fmd encoder on the device (rb2_hip_save_fmd; the arithmetic: rb2_fmd_plan.h; the host side: rb2_engine.hip).
//
// The index is encoded batch by batch.  A batch is an array of run heads rec[] = (global row of the run's first symbol) << 3 | symbol: the runs the
// previous batch could not finish, then the heads found in the next leaves of the piece at hand.  The length of a run is the distance to the
// next head, so the last head of a batch is an open run (until the batch that flushes, which ends with a head at the row count).  From the heads:
//   k_fmds_heads<false/true>  run heads straight from the plane words by neighbour compare: counted per block, then compacted behind a scan
//   k_scan_part/_top/_apply   (rb2_scan.h) W[] = prefix sum of the code widths; the same three launches scan the head counts (sums) and fill the frame
//                             buckets (running maximum)
//   k_fmds_next               for every run i and header type t: where the block that starts at i ends (bisection over W) and the type behind it
//   k_fmds_table              per segment of RB2_FMDS_SEG runs and entry state (run < 96, type): where a walk along next[] leaves it, after how many blocks
//   k_fmds_group              the same for 64 segments: the composition of their tables
//   k_fmds_resolve            one thread walks the groups from the batch's true state; stops where the known runs end, or packs the last block of
//                             a chunk of 2^23 words alone with its shorter tail and ends the batch behind it (the chunk rule is the one thing that
//                             depends on the position in the stream: the tables know nothing of it)
//   k_fmds_down               the true entry state and first block of every segment
//   k_fmds_write              a block per segment: blocks are staged in LDS, 256 at a time and one per thread, and leave as whole lines
//   k_fmds_hdrfix             the header of a segment's first block: the counts of the previous segment's last one
//   k_fmds_carry              the unfinished runs to the front of the next batch's rec[]
//   k_fmds_frames             the rank frames, from the last header of every bucket of rows (kept by k_fmds_write) and one rank query each
// No kernel here uses scratch memory (profiles/fmd_save_resource_usage.txt), and the stream is written without atomics.
#pragma once
#include "rb2_kernels.h"
#include "rb2_query.h"
#include "rb2_fmd_plan.h"

namespace rb2 {

constexpr uint32_t FMDS_GROUP = 64;         // segments per group
constexpr uint32_t FMDS_SEG_MAX = 8192;     // runs per segment at the most: next[] of a segment in LDS
constexpr uint32_t FMDS_DEAD = 0xffffffffu;

struct FmdsState {
	uint64_t m, nc;            // heads in rec[]; complete runs among them: W[0 .. nc], next[0 .. nc]
	uint64_t blk0;             // stream number of the block that starts at run 0 ...
	uint32_t type0, flush;     // ... its header type; the batch holds the last run
	uint64_t nout, carry;      // k_fmds_resolve: blocks the batch emits; first run of the next batch
	uint32_t ctype, done;      // ... the type of the block that starts there; the closing header is among the blocks
	uint32_t cut, err;         // ... the last block is the short one of its chunk; a type-2 header in such a block
	uint64_t cnt[2][7];        // symbols of the last block emitted, by the parity of the batch that needs them
};
struct FmdsEntry { uint32_t off, type; uint64_t blk; };   // a group or a segment: first block start (run, counted from its first run), its type and its number in the batch

// ---- run heads ----------------------------------------------------------------------------------------------------------------------
// one thread per group of 64 symbols of leaves [l0, l0 + nl) of a piece (first leaf leaf0, n symbols, first global row P0)
template <bool WRITE> __global__ __launch_bounds__(256) void k_fmds_heads(PoolView pv, uint64_t leaf0, uint64_t n, uint64_t l0, uint32_t nl, uint64_t P0, uint64_t ncur, uint64_t *rec, uint32_t *wg)
{
	__shared__ uint32_t s_w[4];
	const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	const uint64_t leaf = l0 + (gid >> 4);
	const uint32_t g = (uint32_t)gid & 15u;
	const uint64_t s0 = leaf * LEAF + (uint64_t)g * GSYM;
	uint64_t hm = 0, w0 = 0, w1 = 0, w2 = 0;
	if ((gid >> 4) < nl && s0 < n) {
		const uint64_t *lw = leaf_words(pv.data, leaf0 + leaf);
		w0 = lw[g]; w1 = lw[LEAFG + g]; w2 = lw[2 * LEAFG + g];
		uint64_t q0, q1, q2;                                    // the symbol in front of mine
		if (g > 0) { q0 = lw[g - 1] >> 63; q1 = lw[LEAFG + g - 1] >> 63; q2 = lw[2 * LEAFG + g - 1] >> 63; }
		else if (leaf > 0) { const uint64_t *pw = leaf_words(pv.data, leaf0 + leaf - 1); q0 = pw[LEAFG - 1] >> 63; q1 = pw[2 * LEAFG - 1] >> 63; q2 = pw[3 * LEAFG - 1] >> 63; }
		else if (ncur > 0) { const uint64_t c = rec[ncur - 1] & 7u; q0 = c & 1u; q1 = (c >> 1) & 1u; q2 = c >> 2; }   // the open run of the rows in front of the piece
		else { q0 = ~w0 & 1u; q1 = w1 & 1u; q2 = w2 & 1u; }    // the first row of the index starts a run
		const uint64_t valid = n - s0 >= GSYM ? ~0ull : (1ull << (n - s0)) - 1;
		hm = ((w0 ^ (w0 << 1 | q0)) | (w1 ^ (w1 << 1 | q1)) | (w2 ^ (w2 << 1 | q2))) & valid;
	}
	uint32_t tot;
	const uint32_t ex = block_excl_add<uint32_t>((uint32_t)__popcll(hm), s_w, &tot);
	if (!WRITE) { if (threadIdx.x == 0) wg[blockIdx.x] = tot; return; }
	uint64_t k = ncur + wg[blockIdx.x] + ex;
	while (hm) {
		const uint32_t b = (uint32_t)__builtin_ctzll(hm);
		hm &= hm - 1;
		rec[k++] = (P0 + s0 + b) << 3 | ((w0 >> b) & 1u) | ((w1 >> b) & 1u) << 1 | ((w2 >> b) & 1u) << 2;
	}
}

// the batch as the kernels behind see it: m heads, the closing head behind them when the batch flushes
__global__ void k_fmds_begin(FmdsState *st, uint64_t *rec, uint64_t ncur, const uint32_t *nnew, uint32_t flush, uint64_t total, uint32_t type0, uint64_t blk0)
{
	if (blockIdx.x || threadIdx.x) return;
	const uint64_t m = ncur + (nnew ? *nnew : 0u);
	if (flush) rec[m] = total << 3 | 7u;
	st->m = m; st->nc = flush ? m : (m ? m - 1 : 0);
	st->flush = flush; st->type0 = type0; st->blk0 = blk0;
	st->nout = 0; st->carry = 0; st->ctype = type0; st->done = 0; st->cut = 0;
}

// the code widths of the complete runs, as rb2_scan.h reads an input: their number is known on the device only
struct FmdsInWidth {
	const uint64_t *rec; const FmdsState *st;
	__device__ uint64_t n() const { return st->nc; }
	__device__ uint32_t operator()(uint64_t i) const { return fmds_width((rec[i + 1] >> 3) - (rec[i] >> 3)); }
};

// ---- block boundaries -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fmds_next(const FmdsState *st, const uint64_t *rec, const uint32_t *W, uint32_t *nxt)
{
	const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x, nc = st->nc;
	if (i > nc) return;
	uint32_t v = 0;
#pragma unroll
	for (uint32_t t = 0; t < 3; ++t) {
		if (i == nc) { v |= fmds_next_pack(t, st->flush ? FMDS_FINAL : FMDS_STOP, 0); continue; }
		bool complete;
		uint64_t e = fmds_block_end(W, i, nc, fmds_payload_bits(t, false), &complete);
		if (!complete && !st->flush) { v |= fmds_next_pack(t, FMDS_STOP, 0); continue; }
		v |= fmds_next_pack(t, (uint32_t)(e - i), fmds_type((rec[e] >> 3) - (rec[i] >> 3)));
	}
	nxt[i] = v;
}

// a block per segment, a thread per entry state
__global__ __launch_bounds__(320) void k_fmds_table(const FmdsState *st, const uint32_t *nxt, uint32_t SEG, uint64_t *tab)
{
	__shared__ uint32_t s_n[FMDS_SEG_MAX];
	const uint64_t nc = st->nc, base = (uint64_t)blockIdx.x * SEG;
	if (base > nc) return;
	const uint32_t len = (uint32_t)(nc + 1 - base < SEG ? nc + 1 - base : SEG);
	for (uint32_t k = threadIdx.x; k < len; k += blockDim.x) s_n[k] = nxt[base + k];
	__syncthreads();
	if (threadIdx.x >= FMDS_ENTRIES) return;
	uint32_t r = threadIdx.x / 3, t = threadIdx.x % 3, nb = 0;
	uint64_t x;
	for (;;) {
		if (r >= SEG) { x = fmds_exit_pack(r - SEG, t, 0, nb); break; }
		if (r >= len) { x = fmds_exit_pack(base + r, t, 1, nb); break; }      // (an entry behind the last run: never taken)
		const uint32_t v = s_n[r], d = fmds_next_delta(v, t);
		if (d == FMDS_STOP) { x = fmds_exit_pack(base + r, t, 1, nb); break; }
		if (d == FMDS_FINAL) { x = fmds_exit_pack(base + r, t, 2, nb + 1); break; }
		r += d; t = fmds_next_type(v, t); ++nb;
	}
	tab[(uint64_t)blockIdx.x * FMDS_ENTRIES + threadIdx.x] = x;
}

// the composition of the tables of the segments of a group
__global__ __launch_bounds__(320) void k_fmds_group(const FmdsState *st, const uint64_t *tab, uint32_t SEG, uint64_t *gtab)
{
	const uint64_t nseg = st->nc / SEG + 1, s0 = (uint64_t)blockIdx.x * FMDS_GROUP;
	if (s0 >= nseg || threadIdx.x >= FMDS_ENTRIES) return;
	const uint64_t s1 = s0 + FMDS_GROUP < nseg ? s0 + FMDS_GROUP : nseg;
	uint64_t run = threadIdx.x / 3, nb = 0, x = 0;
	uint32_t t = threadIdx.x % 3, stop = 0;
	for (uint64_t s = s0; s < s1 && !stop; ++s) {
		x = tab[s * FMDS_ENTRIES + run * 3 + t];
		nb += fmds_exit_nblk(x); run = fmds_exit_run(x); t = fmds_exit_type(x); stop = fmds_exit_stop(x);
	}
	gtab[(uint64_t)blockIdx.x * FMDS_ENTRIES + threadIdx.x] = fmds_exit_pack(run, t, stop, nb);
}

// one thread: the true walk over the groups, the end of the batch
__global__ void k_fmds_resolve(FmdsState *st, const uint64_t *rec, const uint32_t *W, const uint32_t *nxt, const uint64_t *tab, const uint64_t *gtab, uint32_t SEG, FmdsEntry *gst)
{
	if (blockIdx.x || threadIdx.x) return;
	const uint64_t nc = st->nc, nseg = nc / SEG + 1, ng = (nseg + FMDS_GROUP - 1) / FMDS_GROUP;
	const uint64_t left = FMDS_CHUNK_BLOCKS - st->blk0 % FMDS_CHUNK_BLOCKS;    // the left-th block of the batch is the last of its chunk
	uint64_t run = 0, cum = 0;
	uint32_t t = st->type0;
	uint64_t g = 0;
	for (; g < ng; ++g) {
		gst[g].off = (uint32_t)run; gst[g].type = t; gst[g].blk = cum;
		const uint64_t x = gtab[g * FMDS_ENTRIES + run * 3 + t], nb = fmds_exit_nblk(x);
		if (cum + nb >= left) {                                 // the short block starts in this group: find it
			uint64_t s = g * FMDS_GROUP;
			for (;; ++s) {
				const uint64_t y = tab[s * FMDS_ENTRIES + run * 3 + t];
				if (cum + fmds_exit_nblk(y) >= left) break;
				cum += fmds_exit_nblk(y); run = fmds_exit_run(y); t = fmds_exit_type(y);
			}
			uint64_t r = s * SEG + run;
			while (cum + 1 < left) { const uint32_t v = nxt[r]; r += fmds_next_delta(v, t); t = fmds_next_type(v, t); ++cum; }
			// (the walk cannot stop on the way: the tables counted these blocks)
			const uint32_t d = fmds_next_delta(nxt[r], t);
			if (d == FMDS_FINAL) { st->nout = left; st->carry = r; st->ctype = t; st->done = 1; }   // the closing header holds no runs: the tail does not matter
			else if (d == FMDS_STOP) { st->nout = left - 1; st->carry = r; st->ctype = t; }
			else {
				if (t == 2) st->err = 1;
				bool complete;
				uint64_t e = fmds_block_end(W, r, nc, fmds_payload_bits(t == 2 ? 1 : t, true), &complete);
				if (!complete && !st->flush) { st->nout = left - 1; st->carry = r; st->ctype = t; }
				else { st->nout = left; st->carry = e; st->ctype = fmds_type((rec[e] >> 3) - (rec[r] >> 3)); st->cut = 1; }
			}
			++g;
			break;
		}
		cum += nb; run = fmds_exit_run(x); t = fmds_exit_type(x);
		if (fmds_exit_stop(x)) { st->nout = cum; st->carry = run; st->ctype = t; st->done = fmds_exit_stop(x) == 2; ++g; break; }
	}
	for (; g < ng; ++g) { gst[g].off = FMDS_DEAD; gst[g].type = 0; gst[g].blk = 0; }
}

// a thread per group: the true entry of its segments
__global__ __launch_bounds__(64) void k_fmds_down(const FmdsState *st, const uint64_t *tab, uint32_t SEG, const FmdsEntry *gst, FmdsEntry *sst)
{
	const uint64_t nseg = st->nc / SEG + 1, g = (uint64_t)blockIdx.x * 64 + threadIdx.x, s0 = g * FMDS_GROUP;
	if (s0 >= nseg) return;
	const uint64_t s1 = s0 + FMDS_GROUP < nseg ? s0 + FMDS_GROUP : nseg, nout = st->nout;
	FmdsEntry e = gst[g];
	bool dead = e.off == FMDS_DEAD;
	for (uint64_t s = s0; s < s1; ++s) {
		if (!dead && e.blk >= nout) dead = true;
		if (dead) { sst[s].off = FMDS_DEAD; sst[s].type = 0; sst[s].blk = 0; continue; }
		sst[s] = e;
		const uint64_t x = tab[s * FMDS_ENTRIES + (uint64_t)e.off * 3 + e.type];
		e.blk += fmds_exit_nblk(x); e.off = (uint32_t)fmds_exit_run(x); e.type = fmds_exit_type(x);
		if (fmds_exit_stop(x)) dead = true;
	}
}

// ---- the blocks ------------------------------------------------------------------------------------------------------------------------
// word W of the header of a block of type `type` whose previous block held c0 symbols, c1 .. c6 of the six (scalars and a constant W: an
// array of counts indexed by a loop variable lands in scratch memory)
template <int W> __device__ __forceinline__ uint64_t fmds_hdrw(uint32_t type, uint64_t c0, uint64_t c1, uint64_t c2, uint64_t c3, uint64_t c4, uint64_t c5, uint64_t c6)
{
	const uint64_t m16 = 0xffffull, m32 = 0xffffffffull;
	const uint64_t t0 = W == 0 ? (c0 & m16) | (c1 & m16) << 16 | (c2 & m16) << 32 | (c3 & m16) << 48 : W == 1 ? (c4 & m16) | (c5 & m16) << 16 | (c6 & m16) << 32 : 0;
	const uint64_t t1 = W == 0 ? (c0 & m32) | c1 << 32 : W == 1 ? (c2 & m32) | c3 << 32 : W == 2 ? (c4 & m32) | c5 << 32 : W == 3 ? (c6 & m32) : 0;
	const uint64_t t2 = W == 0 ? c0 : W == 1 ? c1 : W == 2 ? c2 : W == 3 ? c3 : W == 4 ? c4 : W == 5 ? c5 : c6;
	const uint64_t v = type == 0 ? t0 : type == 1 ? t1 : t2;
	return W == 0 ? v | (uint64_t)type << 62 : v;
}
#define FMDS_HDR_WORDS(type, dst, stride, c0, c1, c2, c3, c4, c5, c6) do { const uint32_t hw_ = fmds_hdr_words(type); \
	(dst)[0] = fmds_hdrw<0>(type, c0, c1, c2, c3, c4, c5, c6); (dst)[stride] = fmds_hdrw<1>(type, c0, c1, c2, c3, c4, c5, c6); \
	if (hw_ > 2) { (dst)[2 * (stride)] = fmds_hdrw<2>(type, c0, c1, c2, c3, c4, c5, c6); (dst)[3 * (stride)] = fmds_hdrw<3>(type, c0, c1, c2, c3, c4, c5, c6); } \
	if (hw_ > 4) { (dst)[4 * (stride)] = fmds_hdrw<4>(type, c0, c1, c2, c3, c4, c5, c6); (dst)[5 * (stride)] = fmds_hdrw<5>(type, c0, c1, c2, c3, c4, c5, c6); \
		(dst)[6 * (stride)] = fmds_hdrw<6>(type, c0, c1, c2, c3, c4, c5, c6); } } while (0)

// A block per segment.  Thread 0 lists the next 256 block starts of the segment along next[]; every thread encodes one of them into its column of
// s_blk (word w of block k at s_blk[w * 256 + k]: a thread's eight words are never an indexed register array) and leaves the block's counts for its
// neighbour, whose header they are; the 256 blocks then leave as 2048 consecutive words, nontemporal.  The header of the segment's FIRST block is
// k_fmds_hdrfix's; lastcnt[s] = the counts of its last one.  bidx/bS: the last header (number, S) of every bucket of 2^bbits rows.
__global__ __launch_bounds__(256) void k_fmds_write(FmdsState *st, const uint64_t *rec, const uint32_t *W, const uint32_t *nxt, const FmdsEntry *sst, uint32_t SEG, int par,
		uint64_t *out, uint64_t *lastcnt, uint64_t *bidx, uint64_t *bS, int bbits)
{
	__shared__ uint64_t s_blk[FMDS_BW * 256];
	__shared__ uint64_t s_cnt[7 * 256];
	__shared__ uint64_t s_prev[7];
	__shared__ uint32_t s_start[257], s_type[256];
	__shared__ uint32_t s_nb, s_more, s_r, s_t;
	const uint64_t s = blockIdx.x, nc = st->nc;
	if (s * SEG > nc) return;
	const FmdsEntry ent = sst[s];
	const uint64_t nout = st->nout, base = s * SEG;
	if (ent.off == FMDS_DEAD || ent.blk >= nout) return;
	const bool cut = st->cut != 0;
	const uint32_t cut_end = (uint32_t)(st->carry - base);     // (only read for the short block)
	if (threadIdx.x == 0) { s_r = ent.off; s_t = ent.type; }
	uint64_t kb = ent.blk;                                      // number (in the batch) of the first block of this round
	bool first = true;
	for (;;) {
		__syncthreads();
		if (threadIdx.x == 0) {
			uint32_t r = s_r, t = s_t, k = 0, more = 1;
			while (k < 256) {
				if (r >= SEG || kb + k >= nout) { more = 0; break; }
				const uint32_t v = nxt[base + r], d = fmds_next_delta(v, t);
				if (d == FMDS_STOP) { more = 0; break; }
				s_start[k] = r; s_type[k] = t | (d == FMDS_FINAL ? 4u : 0u);
				++k;
				if (d == FMDS_FINAL) { more = 0; s_start[k] = r; break; }
				if (cut && kb + k == nout) { s_start[k] = cut_end; more = 0; break; }     // the short block ends where k_fmds_resolve said
				r += d; t = fmds_next_type(v, t);
				s_start[k] = r;
			}
			s_nb = k; s_more = more; s_r = r; s_t = t;
		}
		__syncthreads();
		const uint32_t nb = s_nb, k = threadIdx.x;
		if (nb == 0) break;
		uint64_t c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0, c5 = 0, c6 = 0;
		uint32_t type = 0;
		if (k < nb) {
			type = s_type[k] & 3u;
			const uint64_t i = base + s_start[k], e = base + s_start[k + 1];
			const uint32_t hw = fmds_hdr_words(type), w0 = W[i];
#pragma unroll
			for (uint32_t w = 0; w < FMDS_BW; ++w) s_blk[w * 256 + k] = 0;
			uint64_t p = rec[i];
			for (uint64_t j = i; j < e; ++j) {
				const uint64_t q = rec[j + 1], l = (q >> 3) - (p >> 3);
				const uint32_t a = (uint32_t)p & 7u;
				const FmdsPlace pl = fmds_place(W[j] - w0, fmds_code(l, a), fmds_width(l));
				s_blk[(hw + pl.wi) * 256 + k] |= pl.hi;
				if (pl.spill) s_blk[(hw + pl.wi + 1) * 256 + k] |= pl.lo;
				c0 += l;
				c1 += a == 0 ? l : 0; c2 += a == 1 ? l : 0; c3 += a == 2 ? l : 0; c4 += a == 3 ? l : 0; c5 += a == 4 ? l : 0; c6 += a == 5 ? l : 0;
				p = q;
			}
			s_cnt[k] = c0; s_cnt[256 + k] = c1; s_cnt[512 + k] = c2; s_cnt[768 + k] = c3; s_cnt[1024 + k] = c4; s_cnt[1280 + k] = c5; s_cnt[1536 + k] = c6;
			// the last header of a bucket of rows: the next header (the first of the next batch included) falls into a later one, or there is none
			const uint64_t G = st->blk0 + kb + k, S = rec[i] >> 3, S2 = rec[e] >> 3;
			if (G && bidx && ((s_type[k] & 4u) || (S >> bbits) != (S2 >> bbits))) { bidx[S >> bbits] = G; bS[S >> bbits] = S; }
			if (kb + k + 1 == nout) { uint64_t *d = st->cnt[par ^ 1]; d[0] = c0; d[1] = c1; d[2] = c2; d[3] = c3; d[4] = c4; d[5] = c5; d[6] = c6; }
		}
		__syncthreads();
		if (k < nb && !(first && k == 0)) {
			const uint64_t *q = k ? &s_cnt[k - 1] : s_prev;      // the counts of the block in front: the neighbour's column, or what the last round left
			const uint32_t qs = k ? 256u : 1u;
			const uint64_t p0 = q[0], p1 = q[qs], p2 = q[2 * qs], p3 = q[3 * qs], p4 = q[4 * qs], p5 = q[5 * qs], p6 = q[6 * qs];
			FMDS_HDR_WORDS(type, &s_blk[k], 256, p0, p1, p2, p3, p4, p5, p6);
		}
		__syncthreads();
		if (k == nb - 1) {                                      // (lastcnt every round: the next one may find no block)
			uint64_t *d = lastcnt + s * 7;
			s_prev[0] = d[0] = c0; s_prev[1] = d[1] = c1; s_prev[2] = d[2] = c2; s_prev[3] = d[3] = c3; s_prev[4] = d[4] = c4; s_prev[5] = d[5] = c5; s_prev[6] = d[6] = c6;
		}
		if (out) {
			uint64_t *o = out + kb * FMDS_BW;
#pragma unroll
			for (uint32_t q = 0; q < FMDS_BW; ++q) {
				const uint32_t idx = q * 256 + k;
				if ((idx >> 3) < nb) RB2_STNT(s_blk[(idx & 7u) * 256 + (idx >> 3)], &o[idx]);
			}
		}
		kb += nb; first = false;
		if (!s_more) break;
	}
}

// a thread per segment: the header of its first block
__global__ __launch_bounds__(256) void k_fmds_hdrfix(const FmdsState *st, const FmdsEntry *sst, const uint32_t *nxt, const uint64_t *lastcnt, uint32_t SEG, int par, uint64_t *out)
{
	const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (s * SEG > st->nc) return;
	const FmdsEntry e = sst[s];
	if (e.off == FMDS_DEAD || e.blk >= st->nout) return;
	if (fmds_next_delta(nxt[s * SEG + e.off], e.type) == FMDS_STOP) return;
	const uint64_t *c = s ? lastcnt + (s - 1) * 7 : st->cnt[par];
	const uint64_t c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3], c4 = c[4], c5 = c[5], c6 = c[6];
	FMDS_HDR_WORDS(e.type, out + e.blk * FMDS_BW, 1, c0, c1, c2, c3, c4, c5, c6);
}

// rec[carry .. m] of this batch to the front of the next batch's array (the two take turns)
__global__ __launch_bounds__(256) void k_fmds_carry(const FmdsState *st, const uint64_t *rec, uint64_t *dst)
{
	const uint64_t c = st->carry, n = st->m + 1 - c;
	for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) dst[i] = rec[c + i];
}

// ---- rank frames -------------------------------------------------------------------------------------------------------------------
// frames [f0, f0 + nf), a DPP row of 16 lanes each: frame k >= 1 describes the last header in front of row k << ibits (bidx/bS after their
// prefix maximum: the last header of the buckets up to there), its six counts are one rank query at its S
__global__ __launch_bounds__(256) void k_fmds_frames(const QTab *Tg, PoolView pv, const uint64_t *bidx, const uint64_t *bS, uint64_t nbk, int ibits, int bbits, uint64_t f0, uint64_t nf, uint64_t *out)
{
	__shared__ QTab T;
	qtab_load(Tg, T);
	const QRow R = qrow();
	if (R.i >= nf) return;
	const uint64_t f = f0 + R.i;
	uint64_t idx = 0, S = 0, c6[6] = {0, 0, 0, 0, 0, 0};
	if (f) { const uint64_t j = fmds_frame_last_bucket(f, ibits, bbits, nbk); idx = bidx[j]; S = bS[j]; }
	if (idx) qrank<false>(T, pv, S, c6);
#pragma unroll
	for (uint32_t w = 0; w < 7; ++w)
		if (R.g == w) out[R.i * 7 + w] = w == 0 ? idx * FMDS_BW : QPair<false>::at(c6, (int)w - 1);
}

} // namespace rb2
