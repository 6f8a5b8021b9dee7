// rb2_fmd_load.h -- loader: fermi's .fmd stream (rld0, run-length delta BWT) -> packed leaves of the dense layout.  DESIGN.md section 12.
//
// The stream is cut into blocks of 8 words of 64 bits.  A block begins with a header of 2, 4 or 7 words (type 0, 1, 2 in bits 63-62 of its
// first word: seven u16, u32 or u64) that holds the total and the six symbol counts of the block BEFORE it (rld0.c:107-135); the last
// block of the stream is such a header alone.  Behind the header, runs are coded most-significant bit first, an Elias-delta length and a
// 3-bit symbol each, never across two blocks; the rest of the block is zero.  So every block decodes on its own, one lane per block:
//   k_fmd_sizes   symbols of every block (the total in the NEXT header), summed per group of 256 blocks; header types checked
//   k_scan_block  (rb2_scan.h) exclusive prefix over the groups, in place (one workgroup): the global row of each group's first symbol
//   k_fmd_count   decode every block by count; the six counts checked against the next header; runs cut at the rope boundaries the
//                 file's marginal counts give (the six ropes are concatenated and equal symbols merge across a boundary); the 6 x 6
//                 matrix "symbol a in rope b" tallied in LDS and flushed once per workgroup
//   (host)        piece table and RopeDescs from the matrix, as rb2_hip_load_ropes builds them
//   k_fmd_expand  decode again; global row -> piece through the table of NR + 1 boundaries; symbols ORed into the zeroed pieces with the
//                 group-collecting scheme of k_ld_expand, parts longer than LD_LONG left to k_ld_long; per-piece counts tallied
// A block is decoded by COUNT, from a 64-bit window over its words, until the total of the next header is reached: the shorter payload
// of a block that ends a chunk of 2^23 words (rld0.h:75) and a payload that ends in the block's last bits need no case of their own.
// The window never reads past the block's eight words, whatever the bits say.
#pragma once
#include "rb2_kernels.h"

namespace rb2 {

constexpr int FMD_BW = 8;                                      // words per block (sbits = 3)
constexpr uint32_t FMD_BAD_TYPE  = 1;                          // a header of type 3, or the stream ends inside a header
constexpr uint32_t FMD_BAD_COUNT = 2;                          // a block's symbols disagree with the counts of the next header
constexpr uint32_t FMD_BAD_SYM   = 4;                          // a symbol code above 5
constexpr uint32_t FMD_BAD_TOTAL = 8;                          // more rows than the marginal counts of the file give
struct FmdRopes { uint64_t R[8]; };                            // R[b] = global row of the first symbol of rope b, R[6] = rows, R[7] = ~0
struct FmdPieces {                                             // the NR pieces in global row order: piece p is sub-rope p (rb2_device.h)
	uint64_t q[NR + 1];                                        // global row of the first symbol of piece p (q[NR] = rows)
	uint64_t word0[NR];                                        // first 64-bit word of the piece in the pool
	uint32_t keep[NR];                                         // 0: a piece held by another rank -- counted, not stored
	uint32_t pad;
};

__device__ __forceinline__ uint32_t fmd_hdr_words(uint32_t type) { return type == 0u ? 2u : type == 1u ? 4u : 7u; }
// field i (0 = total, 1..6 = $ACGTN) of the header at h; the type bits sit inside a count field and are masked as rld_rank_index does
// (rld0.c:179-188; a type-0 block holds fewer than 2^14 symbols, a type-1 block fewer than 2^30)
__device__ __forceinline__ uint64_t fmd_hdr_field(const uint64_t *h, uint32_t type, int i)
{
	if (type == 0u) return (h[i >> 2] >> (16 * (i & 3))) & 0x3fffull;
	if (type == 1u) return (h[i >> 1] >> (32 * (i & 1))) & 0x3fffffffull;
	return h[i] & ~(3ull << 62);
}
// the header behind block j (it describes block j): its type, 3 when it is invalid or the stream ends inside it
__device__ __forceinline__ uint32_t fmd_next_type(const uint64_t *w, uint64_t j, uint64_t nwords)
{
	const uint64_t o = (j + 1) * FMD_BW;
	const uint32_t type = (uint32_t)(w[o] >> 62);
	return type < 3u && o + fmd_hdr_words(type) <= nwords ? type : 3u;
}
// the eight words of block j into column t of the workgroup's LDS stage (word k at s_blk[k * 256 + t]: conflict-free for a wave)
__device__ __forceinline__ void fmd_stage_block(const uint64_t *w, uint64_t j, uint64_t *s_col)
{
	const uint4 *p = (const uint4*)(w + j * FMD_BW);           // (the stream is uploaded to an allocation of its own: 64-byte aligned blocks)
#pragma unroll
	for (int k = 0; k < 4; ++k) {
		const uint4 v = p[k];
		s_col[(2 * k) * 256] = (uint64_t)v.y << 32 | v.x;
		s_col[(2 * k + 1) * 256] = (uint64_t)v.w << 32 | v.z;
	}
}
// the runs of one staged block, from bit bp on, until tot symbols are decoded: f(c, l) for each, in order.  Returns 0 or FMD_BAD_*.
// A code is at most 64 bits wide (runs below 2^51), so it lies in one window of 64 bits that starts at its first bit.
template <typename F> __device__ __forceinline__ uint32_t fmd_runs(const uint64_t *s_col, uint32_t bp, uint64_t tot, F f)
{
	while (tot > 0) {
		if (bp >= 64u * FMD_BW) return FMD_BAD_COUNT;          // the payload ran out first
		const uint32_t i = bp >> 6, s = bp & 63u;
		const uint64_t a = s_col[i * 256], b = i + 1 < (uint32_t)FMD_BW ? s_col[(i + 1) * 256] : 0ull;
		const uint64_t win = s ? a << s | b >> (64u - s) : a;
		const uint32_t z = win ? (uint32_t)__builtin_clzll(win) : 64u;   // gamma code of y + 1: z zeros, then y + 1 in z + 1 bits
		if (z > 5u) return FMD_BAD_COUNT;                      // (padding, or not a code of this writer)
		const uint32_t y = (uint32_t)(win >> (63u - 2u * z)) - 1u, wd = 2u * z + 1u + y + 3u;
		if (wd > 64u || bp + wd > 64u * FMD_BW) return FMD_BAD_COUNT;
		const uint64_t v = (win << (2u * z + 1u)) >> (61u - y);  // the low y bits of the length, then the symbol
		const uint64_t l = 1ull << y | v >> 3;
		const uint32_t c = (uint32_t)v & 7u;
		if (c > 5u) return FMD_BAD_SYM;
		if (l > tot) return FMD_BAD_COUNT;                     // overshot
		f(c, l);
		tot -= l; bp += wd;
	}
	return 0;
}

// wg_tot[g] = symbols of blocks [256 g, 256 g + 256)
__global__ __launch_bounds__(256) void k_fmd_sizes(const uint64_t *w, uint64_t nb, uint64_t nwords, uint64_t *wg_tot, uint32_t *bad)
{
	__shared__ uint64_t s_w[4];
	const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	uint64_t n = 0;
	if (j < nb) {
		const uint32_t type = fmd_next_type(w, j, nwords);
		if (type == 3u || (j == 0 && (w[0] >> 62) == 3u)) atomicOr(bad, FMD_BAD_TYPE);
		else n = fmd_hdr_field(w + (j + 1) * FMD_BW, type, 0);
	}
	uint64_t tot;
	block_excl_add<uint64_t>(n, s_w, &tot);
	if (threadIdx.x == 0) wg_tot[blockIdx.x] = tot;
}

// what both decoding passes begin with: stage my block, read the header behind it; returns the bit my payload starts at
__device__ __forceinline__ uint32_t fmd_open_block(const uint64_t *w, uint64_t j, uint64_t nb, uint64_t nwords, uint64_t *s_col, uint64_t &tot, uint32_t &ntype, uint32_t &err)
{
	tot = 0; ntype = 3u;
	if (j >= nb) return 0;
	fmd_stage_block(w, j, s_col);
	const uint32_t type = (uint32_t)(s_col[0] >> 62);
	ntype = fmd_next_type(w, j, nwords);
	if (type == 3u || ntype == 3u) { err |= FMD_BAD_TYPE; ntype = 3u; return 0; }
	tot = fmd_hdr_field(w + (j + 1) * FMD_BW, ntype, 0);
	return 64u * fmd_hdr_words(type);
}

__global__ __launch_bounds__(256) void k_fmd_count(const uint64_t *w, uint64_t nb, uint64_t nwords, const uint64_t *wg_off, FmdRopes ropes, unsigned long long *M /* [6][6] */, uint32_t *bad)
{
	__shared__ uint64_t s_blk[FMD_BW * 256];
	__shared__ uint64_t s_w[4];
	__shared__ uint64_t s_R[8];                                // indexed by the lane's rope cursor
	__shared__ unsigned long long s_m[36];
	if (threadIdx.x < 8) s_R[threadIdx.x] = ropes.R[threadIdx.x];
	if (threadIdx.x < 36) s_m[threadIdx.x] = 0;
	const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	uint64_t tot; uint32_t ntype, err = 0;
	const uint32_t bp = fmd_open_block(w, j, nb, nwords, s_blk + threadIdx.x, tot, ntype, err);
	uint64_t S = wg_off[blockIdx.x] + block_excl_add<uint64_t>(tot, s_w, (uint64_t*)0);   // global row of my first symbol (the barriers also cover s_R, s_m)
	int b = 0;                                                 // rope of S (monotone)
	uint64_t cnt[6] = {0, 0, 0, 0, 0, 0}, lc[6] = {0, 0, 0, 0, 0, 0};   // symbols of my block; those put into rope b so far
	auto tally_out = [&]() {
#pragma unroll
		for (int s = 0; s < 6; ++s) { if (lc[s]) atomicAdd(&s_m[b * 6 + s], (unsigned long long)lc[s]); lc[s] = 0; }
	};
	err |= fmd_runs(s_blk + threadIdx.x, bp, tot, [&](uint32_t c, uint64_t l) {
#pragma unroll
		for (int s = 0; s < 6; ++s) cnt[s] += c == (uint32_t)s ? l : 0ull;   // (no dynamic register indexing)
		while (l > 0) {
			if (b < 6 && S >= s_R[b + 1]) { tally_out(); while (b < 6 && S >= s_R[b + 1]) ++b; }
			if (b >= 6) { err |= FMD_BAD_TOTAL; return; }
			const uint64_t part = min(l, s_R[b + 1] - S);
#pragma unroll
			for (int s = 0; s < 6; ++s) lc[s] += c == (uint32_t)s ? part : 0ull;
			S += part; l -= part;
		}
	});
	if (b < 6) tally_out();
	if (ntype != 3u && !err) {
		const uint64_t *h = w + (j + 1) * FMD_BW;
#pragma unroll
		for (int s = 0; s < 6; ++s) if (cnt[s] != fmd_hdr_field(h, ntype, s + 1)) err |= FMD_BAD_COUNT;
	}
	if (err) atomicOr(bad, err);
	__syncthreads();
	if (threadIdx.x < 36 && s_m[threadIdx.x]) atomicAdd(&M[threadIdx.x], s_m[threadIdx.x]);
}

__global__ __launch_bounds__(256) void k_fmd_expand(const uint64_t *w, uint64_t nb, uint64_t nwords, const uint64_t *wg_off, FmdPieces tab_arg, uint64_t *data,
		unsigned long long *pcnt /* [NR][6] */, LdLong *longs, uint32_t *nlong, uint32_t long_cap, uint32_t *bad)
{
	__shared__ uint64_t s_blk[FMD_BW * 256];
	__shared__ uint64_t s_w[4];
	__shared__ unsigned long long s_pc[NR][6];
	__shared__ FmdPieces tab;                                  // indexed by the lane's piece cursor
	if (threadIdx.x <= NR) tab.q[threadIdx.x] = tab_arg.q[threadIdx.x];
	if (threadIdx.x < NR) { tab.word0[threadIdx.x] = tab_arg.word0[threadIdx.x]; tab.keep[threadIdx.x] = tab_arg.keep[threadIdx.x]; }
	if (threadIdx.x < NR * 6) s_pc[threadIdx.x / 6][threadIdx.x % 6] = 0;
	const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	uint64_t tot; uint32_t ntype, err = 0;
	const uint32_t bp = fmd_open_block(w, j, nb, nwords, s_blk + threadIdx.x, tot, ntype, err);
	uint64_t S = wg_off[blockIdx.x] + block_excl_add<uint64_t>(tot, s_w, (uint64_t*)0);   // global row of my first symbol
	int x = 0;                                                 // piece of S (monotone)
	uint64_t lc[6] = {0, 0, 0, 0, 0, 0};                       // symbols this lane put into piece x so far
	auto tally_out = [&]() {
#pragma unroll
		for (int s = 0; s < 6; ++s) { if (lc[s]) atomicAdd(&s_pc[x][s], (unsigned long long)lc[s]); lc[s] = 0; }
	};
	uint64_t cur_g = ~0ull, cur_w0 = 0, cur_v[3] = {0, 0, 0};  // the group being collected, as in k_ld_expand
	auto flush = [&]() {
		if (cur_g != ~0ull) {
			unsigned long long *q = (unsigned long long*)&data[cur_w0 + (cur_g >> 4) * LEAFW + (cur_g & 15)];
#pragma unroll
			for (int pl = 0; pl < 3; ++pl) if (cur_v[pl]) atomicOr(q + pl * LEAFG, (unsigned long long)cur_v[pl]);
		}
		cur_v[0] = cur_v[1] = cur_v[2] = 0;
	};
	err |= fmd_runs(s_blk + threadIdx.x, bp, tot, [&](uint32_t c, uint64_t l) {
		while (l > 0) {
			if (x < NR && S >= tab.q[x + 1]) { tally_out(); while (x < NR && S >= tab.q[x + 1]) ++x; }
			if (x >= NR) { err |= FMD_BAD_TOTAL; return; }
			const uint64_t part = min(l, tab.q[x + 1] - S), o = S - tab.q[x];
#pragma unroll
			for (int s = 0; s < 6; ++s) lc[s] += c == (uint32_t)s ? part : 0ull;
			if (tab.keep[x] && c != 0) {                       // $ = 0: the pool is zeroed
				if (part > LD_LONG) {
					const uint32_t k = atomicAdd(nlong, 1u);
					if (k < long_cap) { LdLong e; e.word0 = tab.word0[x]; e.o = o; e.n = part; e.c = c; e.pad = 0; longs[k] = e; }
				} else {
					uint64_t gd = o >> 6; uint32_t off = (uint32_t)(o & 63), t = (uint32_t)part;
					while (t > 0) {
						const uint32_t k = min(t, (uint32_t)GSYM - off);
						const uint64_t field = bits_below(k) << off;
						if (gd != cur_g || tab.word0[x] != cur_w0) { flush(); cur_g = gd; cur_w0 = tab.word0[x]; }
						if (c & 1u) cur_v[0] |= field;
						if (c & 2u) cur_v[1] |= field;
						if (c & 4u) cur_v[2] |= field;
						t -= k; off = 0; ++gd;
					}
				}
			}
			S += part; l -= part;
		}
	});
	flush();
	if (x < NR) tally_out();
	if (err) atomicOr(bad, err);
	__syncthreads();
	if (threadIdx.x < NR * 6) {
		const unsigned long long v = s_pc[threadIdx.x / 6][threadIdx.x % 6];
		if (v) atomicAdd(&pcnt[threadIdx.x], v);
	}
}

} // namespace rb2
