// rb2_delete.h -- deleting strings from the device index (rb2_hip_delete_strings).
//
// Removing strings from a multi-string BWT leaves the BWT of the remaining strings: the rows of a string are its LF walk from its row in
// the `$` block, every other row keeps its symbol and its place among the others.  So a deletion is a marking pass and one streaming
// compaction of the flat pieces of the dense layout, pool side to pool side:
//   k_del_mark     one DPP row per id: walk LF from row id to the string's own `$`, set the bit of every row met in a mark word per
//                  source group (indexed like the pool's groups: leaf * 16 + group)
//   k_del_count    one DPP row per source leaf: kept symbols of the leaf; per piece the six kept symbol counts and the removed rows,
//                  tallied in LDS and flushed once per workgroup
//   (host)         piece table and RopeDescs of the survivors from the 31 x 6 matrix, as the loaders build them (ld_piece_table)
//   k_del_scan     one workgroup per piece: exclusive prefix of the kept counts = first destination row of every source leaf (the loop: rb2_scan.h)
//   k_del_compact  one DPP row per source leaf, lane = group: compress the three planes by the kept mask (rb2_delete_plan.h) and OR
//                  them into the zeroed destination piece at the row a row-exclusive sum gives; k_ld_own and the directory follow
// The source is dense and plain (the caller leaves the sparse layout first): row p of a piece is bit p & 63 of group p >> 6.
// Every store and atomic is an ordinary vector one.
#pragma once
#include "rb2_query.h"
#include "rb2_scan.h"
#include "rb2_delete_plan.h"

namespace rb2 {

// the words of the tally: [r * 6 + a] kept symbols a of piece r (what ld_finish reads as the pieces' counts), then per piece the removed
// rows, the source groups that hold rows, those of them that need the compress, and the walk guard
constexpr int DEL_REMOVED = NR * 6, DEL_GROUPS = NR * 7, DEL_SLOW = NR * 7 + 1, DEL_BAD = NR * 7 + 2, DEL_WORDS = NR * 7 + 3;
struct DelPieces { uint64_t leaf0[NR]; };                     // first leaf of every piece on the destination side

// the piece that holds leaf slot gl of the source, -1 for a slot between two pieces
__device__ __forceinline__ int del_piece_of(const QTab &T, uint64_t gl)
{
	int r = -1;
	for (int q = 0; q < NR; ++q) if (gl >= T.rd[q].leaf0 && gl - T.rd[q].leaf0 < T.rd[q].nleaves) r = q;
	return r;
}
// group g of leaf slot gl of piece r: the rows it holds (as a mask)
__device__ __forceinline__ uint64_t del_valid(const RopeDesc &d, uint64_t gl, uint32_t g)
{
	const uint64_t s = ((gl - d.leaf0) << LEAF_SH) + ((uint64_t)g << 6);   // piece row of the group's first symbol
	return s < d.n ? bits_below((uint32_t)min(d.n - s, (uint64_t)GSYM)) : 0ull;
}
__device__ __forceinline__ uint32_t row_incl16(uint32_t v)    // inclusive prefix sum over the 16 lanes of a DPP row (row_shr 1, 2, 4, 8)
{
	v += dpp0<0x111, 0xf>(v); v += dpp0<0x112, 0xf>(v); v += dpp0<0x114, 0xf>(v); v += dpp0<0x118, 0xf>(v);
	return v;
}

// ids[i] < C[1] (the host checked).  A walk that takes more than N steps or leaves the index (an index that is no BWT of complete
// strings) sets *bad and ends; it never ranks or marks a row outside the index.
__global__ __launch_bounds__(256) void k_del_mark(const QTab *Tg, PoolView pv, const int64_t *ids, uint64_t n, unsigned long long *marks, unsigned long long *bad)
{
	__shared__ QTab T;
	qtab_load(Tg, T);
	const QRow R = qrow();
	if (R.i >= n) return;
	const uint64_t N = T.row0[NR];
	uint64_t x = (uint64_t)ids[R.i], steps = 0, c6[6];
	for (;;) {
		const int r = qpiece(T, x);
		const uint64_t p = x - T.row0[r];
		if (R.g == 0) atomicOr(&marks[T.rd[r].leaf0 * LEAFG + (p >> 6)], 1ull << (p & 63));
		if (qlf<false>(T, pv, x, c6) == 0) break;              // the whole-string row: marked, the walk ends
		if (++steps > N || x >= N) { if (R.g == 0) atomicOr(bad, 1ull); break; }
	}
}

__global__ __launch_bounds__(256) void k_del_count(const QTab *Tg, PoolView pv, uint64_t l0, uint64_t nleaf, const unsigned long long *marks, uint32_t *lkept, unsigned long long *tally)
{
	__shared__ QTab T;
	__shared__ unsigned long long s_t[DEL_WORDS];
	if (threadIdx.x < DEL_WORDS) s_t[threadIdx.x] = 0;
	qtab_load(Tg, T);
	const QRow R = qrow();
	const uint64_t gl = l0 + R.i;                          // row i of the launch takes leaf slot l0 + i
	const int r = gl < nleaf ? del_piece_of(T, gl) : -1;
	if (r >= 0) {
		const uint64_t valid = del_valid(T.rd[r], gl, R.g);
		const uint64_t *lw = leaf_words(pv.data, gl);
		const uint64_t mk = marks[gl * LEAFG + R.g], kept = valid & ~mk;
		PlAcc A;
		pl_acc(A, lw[R.g], lw[LEAFG + R.g], lw[2 * LEAFG + R.g], kept);
		const uint32_t r0 = row_sum16(A.p0 | A.p1 << 16), r1 = row_sum16(A.p2 | A.p01 << 16), r2 = row_sum16(A.p02 | (uint32_t)__popcll(valid & mk) << 16);
		const uint32_t r3 = row_sum16((uint32_t)__popcll(kept) | (valid ? 1u << 16 : 0u) | (del_mask_is_prefix(kept) ? 0u : 1u << 24));
		PlAcc S;
		S.p0 = r0 & 0xffffu; S.p1 = r0 >> 16; S.p2 = r1 & 0xffffu; S.p01 = r1 >> 16; S.p02 = r2 & 0xffffu;
		uint32_t c[6];
		pl_finish(S, r3 & 0xffffu, c);
		if (R.g == 0) {
			lkept[gl] = r3 & 0xffffu;
#pragma unroll
			for (int s = 0; s < 6; ++s) if (c[s]) atomicAdd(&s_t[r * 6 + s], (unsigned long long)c[s]);
			if (r2 >> 16) atomicAdd(&s_t[DEL_REMOVED + r], (unsigned long long)(r2 >> 16));
			atomicAdd(&s_t[DEL_GROUPS], (unsigned long long)((r3 >> 16) & 0xffu));
			if (r3 >> 24) atomicAdd(&s_t[DEL_SLOW], (unsigned long long)(r3 >> 24));
		}
	}
	__syncthreads();
	if (threadIdx.x < DEL_WORDS && s_t[threadIdx.x]) atomicAdd(&tally[threadIdx.x], s_t[threadIdx.x]);
}

// workgroup r: lbase[gl] = kept symbols of the leaves of piece r in front of leaf slot gl
__global__ __launch_bounds__(256) void k_del_scan(const QTab *Tg, const uint32_t *lkept, uint64_t *lbase)
{
	__shared__ uint64_t s_w[4];
	const uint64_t leaf0 = Tg->rd[blockIdx.x].leaf0, nl = Tg->rd[blockIdx.x].nleaves;
	uint64_t run = 0;
	scan_by_block<ScanAdd<uint64_t>>(ScanIn<uint32_t>{lkept, 0}, lbase, leaf0, nl, run, s_w);
}

// out: the zeroed data of the destination side.  The host has checked that piece r keeps exactly as many rows as its destination holds.
__global__ __launch_bounds__(256) void k_del_compact(const QTab *Tg, PoolView pv, uint64_t l0, uint64_t nleaf, const unsigned long long *marks, const uint64_t *lbase, DelPieces dst,
                                                     unsigned long long *out)
{
	__shared__ QTab T;
	__shared__ uint64_t s_l0[NR];
	if (threadIdx.x < NR) s_l0[threadIdx.x] = dst.leaf0[threadIdx.x];
	qtab_load(Tg, T);
	const QRow R = qrow();
	const uint64_t gl = l0 + R.i;                          // row i of the launch takes leaf slot l0 + i
	const int r = gl < nleaf ? del_piece_of(T, gl) : -1;
	if (r < 0) return;
	const uint64_t kept = del_valid(T.rd[r], gl, R.g) & ~marks[gl * LEAFG + R.g];
	const uint32_t c = (uint32_t)__popcll(kept);
	const uint64_t d = lbase[gl] + (row_incl16(c) - c);        // destination row of my first kept symbol
	if (c == 0) return;
	const uint64_t *lw = leaf_words(pv.data, gl);
	uint64_t v[3] = { lw[R.g], lw[LEAFG + R.g], lw[2 * LEAFG + R.g] };
	if (del_mask_is_prefix(kept)) {                            // nothing to close up inside the group: the common case when few strings go
#pragma unroll
		for (int pl = 0; pl < 3; ++pl) v[pl] &= kept;
	} else {
		const DelCompress P = del_compress_plan(kept);
#pragma unroll
		for (int pl = 0; pl < 3; ++pl) v[pl] = del_compress(P, v[pl]);
	}
#pragma unroll
	for (int pl = 0; pl < 3; ++pl) {
		if (!v[pl]) continue;                                  // (`$` is 000 and the pool is zeroed)
		const DelDst D = del_dst(s_l0[r], d, c, (uint32_t)pl);
		atomicOr(out + D.word, (unsigned long long)(v[pl] << D.shift));
		if (D.spill && (v[pl] >> (64u - D.shift))) atomicOr(out + D.word2, (unsigned long long)(v[pl] >> (64u - D.shift)));
	}
}

} // namespace rb2
