// rb2_query.h -- FM-index queries on the device index: backward search, bi-interval extension (rld_extend), inverse BWT.
//
// Coordinates (include/rb2_hip.h): global rows run over the concatenated BWT, rope 0 ($) .. rope 5 (N); rope b is its pieces (b,$) ..
// (b,N) in index order, so the sub-rope numbers r = 0 .. NR-1 are already the order of the rows.  C[a] = rows in front of rope a.
//
// The one primitive is the GLOBAL RANK qrank(): the six counts in front of a global row.  A per-launch table (QTab, built by k_qtab from
// ctl->rope[side] on the device, copied to LDS by every block) gives each piece its first row, the counts of the rows in front of it and
// sb_cum() of its first superblock; qrank() finds the piece of the row, ranks inside it exactly as wave_rank_all does (dense: leaf =
// p >> 10 and LeafMeta; sparse: locate(), the directory prefix, two-plane leaves) and adds the piece's counts in front.
//
// One query = one DPP row of 16 lanes, four queries per wave: lane g of the row reads group g of the leaf (three coalesced 128-byte
// lines per row), popcounts its share of [0, off) and the row sums the packed counts with four row_ror steps, so every lane of the row
// ends up with the six counts (wave_rank_all spends a whole wave on one query and leaves 48 lanes idle).  All 16 lanes of a row carry the
// same query and take the same branches; different rows of a wave diverge freely (the DPP moves never leave a row).
// Queries read the pool, the directory and ctl->rope only: they never write the index, the Ctl or a buffer an insert reads.
#pragma once
#include "rb2_device.h"
#include "rb2_kmer_plan.h"
#include "rb2_query_plan.h"

namespace rb2 {

struct QTab {
	uint64_t row0[NR + 1];     // first global row of piece r; [NR] = N, the number of rows
	uint64_t pre[NR][6];       // symbol counts of the global rows in front of piece r
	uint64_t sbc[NR][6];       // sb_cum(pv, rope[r].sb0, a) (0 for an empty piece)
	RopeDesc rd[NR];           // ctl->rope[side]
};

// the table of the current index: one thread per piece copies its descriptor and reads its sb_cum(), thread 0 sums the rows and counts
__global__ void k_qtab(const Ctl *ctl, int side, PoolView pv, QTab *T)
{
	const int r = (int)threadIdx.x;
	if (blockIdx.x != 0) return;
	if (r < NR) {
		const RopeDesc d = ctl->rope[side][r];
		T->rd[r] = d;
		for (int a = 0; a < 6; ++a) T->sbc[r][a] = d.nleaves ? sb_cum(pv, d.sb0, a) : 0;
	}
	if (r != 0) return;
	uint64_t row = 0, pre[6] = {0, 0, 0, 0, 0, 0};
	for (int q = 0; q < NR; ++q) {
		const RopeDesc &d = ctl->rope[side][q];
		T->row0[q] = row;
		for (int a = 0; a < 6; ++a) { T->pre[q][a] = pre[a]; pre[a] += d.cnt[a]; }
		row += d.n;
	}
	T->row0[NR] = row;
}

// block prologue of every query kernel: the table to LDS
__device__ __forceinline__ void qtab_load(const QTab *g, QTab &s)
{
	const uint32_t *src = (const uint32_t*)g; uint32_t *dst = (uint32_t*)&s;
	for (uint32_t i = threadIdx.x; i < sizeof(QTab) / 4; i += blockDim.x) dst[i] = src[i];
	__syncthreads();
}

__device__ __forceinline__ uint32_t row_sum16(uint32_t v)     // sum over the 16 lanes of a DPP row, in every lane of it (row_ror 8, 4, 2, 1)
{
	v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, false);
	v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xf, 0xf, false);
	v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x122, 0xf, 0xf, false);
	v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x121, 0xf, 0xf, false);
	return v;
}

// the piece that holds global row x (x < N), or the last piece for x == N: the last r with row0[r] <= x -- a piece that holds x when
// x < N (empty pieces share their first row with the next one)
__device__ __forceinline__ int qpiece(const QTab &T, uint64_t x)
{
	int lo = 0, hi = NR - 1;
	while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (T.row0[mid] <= x) lo = mid; else hi = mid - 1; }
	return lo;
}

// occ(a, x) for all six a (x <= N); *sym (if asked, x < N): the symbol at row x.  All 16 lanes of the row call it with the same x.
template <bool SPARSE> __device__ inline void qrank(const QTab &T, const PoolView &pv, uint64_t x, uint64_t out[6], uint32_t *sym = nullptr)
{
	const int r = qpiece(T, x);
	const RopeDesc &rp = T.rd[r];
	const uint64_t p = x - T.row0[r];
	if (p >= rp.n) {
#pragma unroll
		for (int s = 0; s < 6; ++s) out[s] = T.pre[r][s] + rp.cnt[s];
		return;
	}
	uint64_t gl; uint32_t off; bool p2 = true;
	if (SPARSE) { const Loc lc = locate(pv, rp, p); gl = lc.gl; off = (uint32_t)(p - lc.s); p2 = lc.p2 != 0; }
	else { gl = rp.leaf0 + (p >> LEAF_SH); off = (uint32_t)(p & (LEAF - 1)); }
	const uint32_t g = (uint32_t)lane_id() & 15u, b = g << 6;
	const uint64_t *lw = leaf_words(pv.data, gl);
	const uint64_t b0 = lw[g], b1 = lw[LEAFG + g], b2 = leaf_p2(p2, b0, b1, p2 ? lw[2 * LEAFG + g] : 0);
	PlAcc A;
	pl_acc(A, b0, b1, b2, off > b ? bits_below(min(off - b, 64u)) : 0ull);
	uint32_t sv = 0;
	if (sym && (off >> 6) == g) { const uint32_t k = off & 63u; sv = (uint32_t)((b0 >> k) & 1u) | (uint32_t)((b1 >> k) & 1u) << 1 | (uint32_t)((b2 >> k) & 1u) << 2; }
	const uint32_t r0 = row_sum16(A.p0 | A.p1 << 16), r1 = row_sum16(A.p2 | A.p01 << 16), r2 = row_sum16(A.p02 | sv << 16);
	PlAcc S;
	S.p0 = r0 & 0xffffu; S.p1 = r0 >> 16; S.p2 = r1 & 0xffffu; S.p01 = r1 >> 16; S.p02 = r2 & 0xffffu;
	if (sym) *sym = r2 >> 16;
	uint32_t c[6];
	pl_finish(S, off, c);
	uint32_t pc[6];                                            // the leaves of the superblock in front of this one
	if (SPARSE) {
#pragma unroll
		for (int s = 0; s < 6; ++s) pc[s] = dir_prefix(pv, gl / SB, 1 + s, (uint32_t)(gl % SB));
	} else {
		const LeafMeta m = pv.meta[gl];
#pragma unroll
		for (int s = 0; s < 6; ++s) pc[s] = m.c[s];
	}
#pragma unroll
	for (int s = 0; s < 6; ++s) out[s] = T.pre[r][s] + (sb_cum(pv, gl / SB, s) - T.sbc[r][s]) + pc[s] + c[s];
}

__device__ __forceinline__ uint64_t qC(const QTab &T, int a) { return T.row0[rope_of(a, 0)]; }   // C[a]: rows in front of rope a

constexpr int QPB = 256 / 16;              // queries per block of 256 threads

// ---- what the row kernels are made of: each kernel below is these helpers plus its own loop ----

// the DPP row of this thread: i = its number in the launch (the item it takes), b = the number of the block's first row (the same in the
// whole block), g = the lane inside the row
struct QRow { uint64_t b, i; uint32_t g; };
__device__ __forceinline__ QRow qrow()
{
	const uint64_t b = (uint64_t)blockIdx.x * QPB;
	return {b, b + (threadIdx.x >> 4), (uint32_t)lane_id() & 15u};
}

// the ranks at the two ends of an interval [lo, hi) (lo <= hi <= N): cl[a] = occ(a, lo), ch[a] = occ(a, hi).  size(a) = the rows of the
// interval whose symbol is a (size(0): the whole strings among them, in front of which stand cl[0] others); child(c) = the interval of c
// followed by the word of [lo, hi), empty (nlo >= nhi) when that word does not occur
template <bool SPARSE> struct QPair {
	uint64_t cl[6], ch[6];
	__device__ __forceinline__ QPair() {}
	__device__ __forceinline__ QPair(const QTab &T, const PoolView &pv, uint64_t lo, uint64_t hi) { qrank<SPARSE>(T, pv, lo, cl); qrank<SPARSE>(T, pv, hi, ch); }
	static __device__ __forceinline__ uint64_t at(const uint64_t (&v)[6], int a)   // v[a] by selects: an index into a member the compiler does not know puts the pair into scratch
	{
		const uint64_t v0 = v[0], v1 = v[1], v2 = v[2], v3 = v[3], v4 = v[4], v5 = v[5];
		return a == 0 ? v0 : a == 1 ? v1 : a == 2 ? v2 : a == 3 ? v3 : a == 4 ? v4 : v5;
	}
	__device__ __forceinline__ uint64_t size(int a) const { return at(ch, a) - at(cl, a); }
	template <typename I> __device__ __forceinline__ void child(const QTab &T, int c, I &nlo, I &nhi) const { const uint64_t C = qC(T, c); nlo = (I)(C + at(cl, c)); nhi = (I)(C + at(ch, c)); }
};

// The kid line: entry e of a path stack (k_approx, k_approx_ed, k_irreducible; DESIGN.md section 16, "the path stack") is the 64 bytes
// kid[8 e + 2 (a - 1) ..] = lo, hi of the children a = 1 .. 4 of a ranked interval.  Lanes 0 .. 7 of the row store one word each and all
// sixteen read: the vector memory operations of one wave are performed in order, and two fences keep the compiler from moving them --
// the release fence behind the store is kid_store's, the acquire fence in front of a read is the caller's, once for all it reads next.
// kid_store: klo, khi = the children of P, written as line e (g = the lane of the row)
template <bool SPARSE> __device__ __forceinline__ void kid_store(const QTab &T, const QPair<SPARSE> &P, uint64_t *kid, int64_t e, uint32_t g, uint64_t (&klo)[4], uint64_t (&khi)[4])
{
	uint64_t v = 0;
#pragma unroll
	for (int a = 1; a <= 4; ++a) P.child(T, a, klo[a - 1], khi[a - 1]);
#pragma unroll
	for (int w = 0; w < 8; ++w) if (g == (uint32_t)w) v = w & 1 ? khi[w >> 1] : klo[w >> 1];
	if (g < 8) kid[8 * e + g] = v;
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
}
// child a of line e
__device__ __forceinline__ void kid_child(const uint64_t *kid, int64_t e, int a, uint64_t &lo, uint64_t &hi) { lo = kid[8 * e + 2 * (a - 1)]; hi = kid[8 * e + 2 * (a - 1) + 1]; }
// all four children of line e
__device__ __forceinline__ void kid_line(const uint64_t *kid, int64_t e, uint64_t (&klo)[4], uint64_t (&khi)[4])
{
#pragma unroll
	for (int c = 0; c < 4; ++c) kid_child(kid, e, c + 1, klo[c], khi[c]);
}

// one LF step from row x (x < N): returns the symbol c of the row and, unless it is `$`, moves x to the row of the suffix one longer;
// c6 = the counts in front of the row x was (c6[0]: the `$`s in front of it, which names the string when c is `$`).  On an index that
// is no BWT of complete strings the new x can be N or more and a walk need not end: the guard is the caller's, because the three differ.
// k_ssa_build and k_locate count their steps against N and test x < N after every step, so they never rank a row outside the index;
// k_extract has no guard and relies on max_len to end (for a row that is not there qrank reads no memory and leaves the symbol unset).
template <bool SPARSE> __device__ __forceinline__ uint32_t qlf(const QTab &T, const PoolView &pv, uint64_t &x, uint64_t c6[6])
{
	uint32_t c;
	qrank<SPARSE>(T, pv, x, c6, &c);
	if (c != 0) x = qC(T, (int)c) + c6[c];
	return c;
}

// query i of a packed batch: q[0 .. L) = qry[off[i] - base, off[i + 1] - base).  bad: the offsets are no slice (or the caller says so:
// bad0), or a symbol is no code 1 .. 5; with END0 a 0 (`$`) may stand as the last symbol.  The symbols of a bad slice are not all read.
struct QSlice { const uint8_t *q; int64_t L; bool bad; };
template <bool END0> __device__ __forceinline__ QSlice qslice(const uint8_t *qry, const int64_t *off, int64_t base, uint64_t i, bool bad0 = false)
{
	const int64_t s0 = off[i] - base, L = off[i + 1] - base - s0;
	QSlice S = {qry + s0, L, bad0 || L < 0 || s0 < 0};
	for (int64_t j = 0; !S.bad && j < L; ++j) { const uint8_t c = S.q[j]; S.bad = c > 5 || (c == 0 && !(END0 && j == L - 1)); }
	return S;
}

// record k of item i, the W words v... at rec[(i * cap + k) * W ..], stored by the lanes g < W of the row (lane g stores the g-th word:
// one store of 8 W bytes) when k < cap; a record beyond cap is the caller's to count
template <typename... V> __device__ __forceinline__ void qstore(int64_t *rec, uint64_t i, int64_t cap, int64_t k, uint32_t g, V... v)
{
	constexpr uint32_t W = sizeof...(V);
	if (k >= cap || g >= W) return;
	int64_t x = 0;
	uint32_t w = 0;
	((x = g == w++ ? (int64_t)v : x), ...);
	rec[(i * (uint64_t)cap + (uint64_t)k) * W + g] = x;
}

// slot q of a launch that takes kn hits of each of n ranges, from hit k0 on (kn = max_hits and k0 = 0 unless one range alone has more
// slots than a launch takes: split_slots): hit kk = k0 + q % kn of range i = q / kn, [lo, hi) = rv[2i ..] inside [0, top].  The slot of
// hit 0 writes cnt[i] = hi - lo, -1 for a malformed range (if it is the `writer`: one lane of a row).  live: the slot has a hit, x = lo + kk
struct QSlot { uint64_t i; int64_t kk, x; bool live; };
__device__ __forceinline__ QSlot qslot(uint64_t q, uint64_t n, int64_t k0, int64_t kn, const int64_t *rv, int64_t top, bool writer, int64_t *cnt)
{
	if (q >= n * (uint64_t)kn) return {0, 0, 0, false};
	const uint64_t i = q / (uint64_t)kn;
	const int64_t kk = k0 + (int64_t)(q % (uint64_t)kn), lo = rv[2 * i], hi = rv[2 * i + 1];
	const bool bad = lo < 0 || hi > top || lo > hi;
	if (kk == 0 && writer) cnt[i] = bad ? -1 : hi - lo;
	return {i, kk, lo + kk, !bad && kk < hi - lo};
}

// backward search: n patterns pat[off[i] - base, off[i+1] - base), out[3i..] = lo, hi, m (include/rb2_hip.h)
template <bool SPARSE> __global__ __launch_bounds__(256) void k_bsearch(const QTab *Tg, PoolView pv, const uint8_t *pat, const int64_t *off, int64_t base,
                                                                        uint64_t n, int64_t *out)
{
	__shared__ QTab T;
	qtab_load(Tg, T);
	const QRow R = qrow();
	if (R.i >= n) return;
	const QSlice S = qslice<true>(pat, off, base, R.i);
	int64_t lo = 0, hi = (int64_t)T.row0[NR], m = 0;
	if (S.bad) lo = hi = m = -1;
	else {
		for (int64_t j = S.L - 1; j >= 0; --j) {
			uint64_t nl, nh;
			QPair<SPARSE>(T, pv, (uint64_t)lo, (uint64_t)hi).child(T, S.q[j], nl, nh);
			if (nl >= nh) break;                               // the suffix one longer does not occur: stop early
			lo = (int64_t)nl; hi = (int64_t)nh; ++m;
		}
	}
	qstore(out, R.i, 1, 0, R.g, lo, hi, m);
}

// rld_extend (rld0.c:474-490) on n bi-intervals: ok[18i + 3a + j]
template <bool SPARSE> __global__ __launch_bounds__(256) void k_extend(const QTab *Tg, PoolView pv, const int64_t *ik, int is_back, uint64_t n, int64_t *ok)
{
	__shared__ QTab T;
	qtab_load(Tg, T);
	const QRow R = qrow();
	if (R.i >= n) return;
	const int fb = !is_back;
	const uint64_t x0 = (uint64_t)ik[3 * R.i + fb], sz = (uint64_t)ik[3 * R.i + 2], xb = (uint64_t)ik[3 * R.i + is_back];
	QPair<SPARSE> P;                                                 // (an empty interval needs one rank only)
	qrank<SPARSE>(T, pv, x0, P.cl);
	if (sz) qrank<SPARSE>(T, pv, x0 + sz, P.ch);
	else for (int a = 0; a < 6; ++a) P.ch[a] = P.cl[a];
	int64_t xf[6], sz6[6], xo[6];                              // x[!is_back], x[2], x[is_back] of the six extensions
#pragma unroll
	for (int a = 0; a < 6; ++a) { int64_t xh; P.child(T, a, xf[a], xh); sz6[a] = (int64_t)P.size(a); }
	xo[0] = (int64_t)xb;                                       // the other end in the complement order $ T G C A N
	xo[4] = xo[0] + sz6[0];
	xo[3] = xo[4] + sz6[4];
	xo[2] = xo[3] + sz6[3];
	xo[1] = xo[2] + sz6[2];
	xo[5] = xo[1] + sz6[1];
#pragma unroll
	for (int k = 0; k < 18; ++k)                               // 18 words: lanes 0..15, then lanes 0..1 again
		if ((uint32_t)(k & 15) == R.g) ok[18 * R.i + k] = k % 3 == 2 ? sz6[k / 3] : k % 3 == fb ? xf[k / 3] : xo[k / 3];
}

// inverse BWT from rows of the $ block: the string of row rows[i], LAST symbol first, into out[i * max_len ..) (the host reverses it);
// len[i] = its length, -1 when longer than max_len, -2 for a row outside [0, C[1])
template <bool SPARSE> __global__ __launch_bounds__(256) void k_extract(const QTab *Tg, PoolView pv, const int64_t *rows, uint64_t n, int64_t max_len,
                                                                        uint8_t *out, int64_t *len)
{
	__shared__ QTab T;
	qtab_load(Tg, T);
	const QRow R = qrow();
	if (R.i >= n) return;
	const int64_t row = rows[R.i];
	int64_t k = 0;
	if (row < 0 || (uint64_t)row >= qC(T, 1)) k = -2;
	else {
		uint64_t x = (uint64_t)row;
		uint8_t *o = out + R.i * (uint64_t)max_len;
		for (;;) {
			uint64_t c6[6];
			const uint32_t c = qlf<SPARSE>(T, pv, x, c6);
			if (c == 0) break;                                 // back at the string's own '$' row
			if (k == max_len) { k = -1; break; }
			if (R.g == 0) o[k] = (uint8_t)c;
			++k;
		}
	}
	if (R.g == 0) len[R.i] = k;
}

// super-maximal exact matches of n queries qry[off[i] - base, off[i+1] - base) (codes 1..4 match, 5 belongs to no match, anything else
// makes the query malformed) against an index that holds both strands: records (start, end, x0, x1, size) in increasing start into
// mem[(i * max_mems + k) * 5 ..) for k < max_mems, cnt[i] = SMEMs found (the surplus is counted, not stored), -1 for a malformed query.
//
// If the previous SMEM ended at p, the next one is the match with the smallest start among those that cover position p: from the
// bi-interval of q[p] extend backward while size >= min_occ (that gives its start s), then forward from p + 1 (that gives e(s)), and go
// on from p = e(s).  A start between the previous one and s cannot begin an SMEM: it would cover p with a smaller start.  A position
// whose symbol alone has fewer than min_occ occurrences is skipped.  p grows by at least 1 per turn, so the loop ends whatever the index
// holds; steps <= sum of the SMEM lengths + L.  The state is one bi-interval as (xf, xo, sz): xf = the end the next step ranks (x0 going
// backward, x1 going forward), so turning round is a swap and both directions share one step, the arithmetic of k_extend for one symbol.
// Left alone the compiler takes 108-114 VGPRs (4 waves per SIMD) to overlap the two ranks of a step; held to 5 waves it needs 90-93 and
// still no scratch (6 waves would spill).
template <bool SPARSE> __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 5))) void k_smem(const QTab *Tg, PoolView pv, const uint8_t *qry, const int64_t *off, int64_t base,
                                                                     uint64_t n, int64_t min_len, int64_t min_occ, int64_t max_mems, int64_t *mem, int64_t *cnt)
{
	__shared__ QTab T;
	qtab_load(Tg, T);
	const QRow R = qrow();
	if (R.i >= n) return;
	const QSlice S = qslice<false>(qry, off, base, R.i);
	if (S.bad) { if (R.g == 0) cnt[R.i] = -1; return; }
	const int64_t L = S.L, N = (int64_t)T.row0[NR];
	int64_t k = 0, p = 0;
	while (p < L) {
		const int c0 = S.q[p];
		int64_t xf = (int64_t)qC(T, c0 < 5 ? c0 : 0), xo = (int64_t)qC(T, c0 < 5 ? 5 - c0 : 0), sz = c0 < 5 ? (int64_t)qC(T, c0 + 1) - xf : 0;
		if (sz < min_occ) { ++p; continue; }                       // N, or a symbol with too few occurrences: no match covers p
		int64_t s = p, e = p + 1;
		bool back = true;
		for (;;) {
			const int64_t j = back ? s - 1 : e;
			const int c = j >= 0 && j < L ? S.q[j] : 0;
			bool stop = c < 1 || c > 4;
			if (!stop) {
				const int a = back ? c : 5 - c;                    // a forward extension by c is the extension of the other strand by its complement
				const QPair<SPARSE> P(T, pv, (uint64_t)min(max(xf, (int64_t)0), N), (uint64_t)min(max(xf + sz, (int64_t)0), N));
				const int64_t nsz = (int64_t)P.size(a);
				if (nsz < min_occ) stop = true;
				else {
					xo += (int64_t)P.size(0);                      // the other end in the complement order $ T G C A N
#pragma unroll
					for (int b = 4; b >= 2; --b) if (b > a) xo += (int64_t)P.size(b);
					int64_t xh;
					P.child(T, a, xf, xh); sz = nsz;
					if (back) --s; else ++e;
				}
			}
			if (stop) {
				if (!back) break;
				back = false;
				const int64_t t = xf; xf = xo; xo = t;
			}
		}
		if (e - s >= min_len) { qstore(mem, R.i, max_mems, k, R.g, s, e, xo, xf, sz); ++k; }
		p = e;
	}
	if (R.g == 0) cnt[R.i] = k;
}

// ---- sampled suffix array ----
// String k = row k of the $ block; its walk x_0 = k, x_{j+1} = LF(x_j) ends at the first row whose symbol is `$`, after len[k] steps.
// Row x_j is the suffix of string k that starts j symbols before its end: SA(x_j) = (k, len[k] - j).  The walks are the cycles of LF cut
// at the `$`s, so every row lies on exactly one walk and every slot below is written by exactly one string: no atomics.
//   smp[2 * (x >> s) ..] = k, j    for the rows x with x % 2^s == 0 (two 64-bit words: ids go up to n, distances up to 2^48)
//   slen[k] = len[k]               head[q] = k for the q-th whole-string row (q = the `$`s in front of the row where the walk of k ends)
// A walk is cut off after N steps and an index out of range is not stored: an index that is no BWT of complete strings (load_ropes takes
// any six streams with consistent totals) then gives a wrong array, never a write out of bounds or a kernel that does not end.

// the walks of strings k0 .. n - 1 (n = C[1]) as far as the launch reaches, one string per DPP row
template <bool SPARSE> __global__ __launch_bounds__(256) void k_ssa_build(const QTab *Tg, PoolView pv, uint64_t k0, uint64_t n, int s, uint64_t *smp, uint64_t *slen, uint64_t *head)
{
	__shared__ QTab T;
	qtab_load(Tg, T);
	const QRow R = qrow();
	const uint64_t k = k0 + R.i;
	if (k >= n) return;
	const uint64_t N = T.row0[NR], mask = (1ull << s) - 1;
	uint64_t x = k, j = 0, c6[6];
	for (;;) {
		if ((x & mask) == 0) qstore((int64_t*)smp, x >> s, 1, 0, R.g, k, j);   // (one sample is one record)
		if (qlf<SPARSE>(T, pv, x, c6) == 0 || j >= N) break;
		++j;
		if (x >= N) break;
	}
	if (R.g == 0) { slen[k] = j; if (c6[0] < n) head[c6[0]] = k; }
}

// rows to places: slot q of the launch is hit kk of interval i (qslot).  The row lo_i + kk walks LF, counting its
// steps t, to the first row that is a sample (sid, j): (sid, len[sid] - j + t) -- or whose symbol is `$`: (head[`$`s in front], t).  The
// sample is tested first, so the rows of the $ block need no case of their own: row k < n is step 0 of the walk of string k, and what the
// walk from it meets -- a sample of string k at step j (t = j) or the end of string k (t = len[k]) -- gives (k, len[k]) either way.
// hit[(i * max_hits + kk) * 2 ..] = string, position; cnt[i] = hi - lo, -1 for a malformed interval.
template <bool SPARSE> __global__ __launch_bounds__(256) void k_locate(const QTab *Tg, PoolView pv, const int64_t *iv, uint64_t n, int64_t max_hits, int64_t k0, int64_t kn,
                                                                       int s, const uint64_t *smp, const uint64_t *slen, const uint64_t *head, uint64_t nstr,
                                                                       int64_t *hit, int64_t *cnt)
{
	__shared__ QTab T;
	qtab_load(Tg, T);
	const QRow R = qrow();
	const uint64_t N = T.row0[NR], mask = (1ull << s) - 1;
	const QSlot S = qslot(R.i, n, k0, kn, iv, (int64_t)N, R.g == 0, cnt);
	if (!S.live) return;
	uint64_t x = (uint64_t)S.x, t = 0, sid = 0, pos = 0;
	for (;;) {
		if ((x & mask) == 0) {
			sid = smp[2 * (x >> s)];
			pos = (sid < nstr ? slen[sid] : 0) - smp[2 * (x >> s) + 1] + t;
			break;
		}
		uint64_t c6[6];
		if (qlf<SPARSE>(T, pv, x, c6) == 0) { sid = c6[0] < nstr ? head[c6[0]] : 0; pos = t; break; }
		if (++t > N || x >= N) break;                              // (no BWT of complete strings)
	}
	qstore(hit, S.i, max_hits, S.kk, R.g, sid, pos);
}

// ---- suffix-prefix overlaps ----
// A row of the interval [lo, hi) of a pattern P, |P| >= 1, whose BWT symbol is `$` is the row of a whole string that starts with P.  So
// occ($, hi) - occ($, lo) strings have the prefix P, and they are head[q] (the array k_ssa_build writes) for q in [occ($, lo), occ($, hi)).

// backward search of n queries qry[off[i] - base, off[i+1] - base) (codes 1..4 match, 5 ends the search, anything else makes the query
// malformed) that reports on its way every suffix some string of the index starts with: records (l, zlo, zhi) in increasing l into
// rec[(i * max_recs + k) * 3 ..) for k < max_recs, cnt[i] = records found (the surplus is counted, not stored), -1 for a malformed query.
// The pair of ranks at the two ends of the interval of the last m symbols serves twice: the `$` counts are the record of length m, the
// counts of the next symbol are the step.  The search starts at the interval of the last symbol (C[c], C[c + 1]: no rank) and ends
// behind the ranks of the whole query, at an N, or when the interval empties: at most len rank pairs.
template <bool SPARSE> __global__ __launch_bounds__(256) void k_overlap(const QTab *Tg, PoolView pv, const uint8_t *qry, const int64_t *off, int64_t base,
                                                                        uint64_t n, int64_t min_ovlp, int64_t max_recs, int64_t *rec, int64_t *cnt)
{
	__shared__ QTab T;
	qtab_load(Tg, T);
	const QRow R = qrow();
	if (R.i >= n) return;
	const QSlice S = qslice<false>(qry, off, base, R.i);
	if (S.bad) { if (R.g == 0) cnt[R.i] = -1; return; }
	const int c0 = S.L > 0 ? S.q[S.L - 1] : 5;
	int64_t lo = (int64_t)qC(T, c0 < 5 ? c0 : 0), hi = c0 < 5 ? (int64_t)qC(T, c0 + 1) : lo, m = 1, k = 0;
	while (lo < hi) {
		const QPair<SPARSE> P(T, pv, (uint64_t)lo, (uint64_t)hi);
		if (m >= min_ovlp && P.ch[0] > P.cl[0]) { qstore(rec, R.i, max_recs, k, R.g, m, P.cl[0], P.ch[0]); ++k; }
		if (m == S.L) break;
		const int c = S.q[S.L - 1 - m];
		if (c == 5) break;
		P.child(T, c, lo, hi); ++m;
	}
	if (R.g == 0) cnt[R.i] = k;
}

// `$` ranks to string ids: slot q of the launch is hit kk of range i (qslot; covered in parts as k_locate is), one thread
// per slot, so a range reads head[] and writes ids[] in whole lines.  ids[i * max_hits + kk] = head[zlo_i + kk]; cnt[i] = zhi - zlo, -1
// for a malformed range.
__global__ __launch_bounds__(256) void k_string_ids(const int64_t *zv, uint64_t n, int64_t max_hits, int64_t k0, int64_t kn, const uint64_t *head, uint64_t nstr,
                                                    int64_t *ids, int64_t *cnt)
{
	const QSlot S = qslot((uint64_t)blockIdx.x * 256 + threadIdx.x, n, k0, kn, zv, (int64_t)nstr, true, cnt);
	if (S.live) ids[S.i * (uint64_t)max_hits + (uint64_t)S.kk] = (int64_t)head[S.x];
}

// ---- k-mer enumeration ----
// The two ranks of an interval [lo, hi) give the intervals of all four one-symbol left extensions at once: the child of the l-mer P by a
// is aP = [C[a] + occ(a, lo), C[a] + occ(a, hi)), and aP cannot occur more often than P, so a child smaller than min_occ is dropped for
// good.  From the single item (0, 0, N) -- the empty word -- k levels of that give every k-mer with at least min_occ occurrences, each once.

constexpr int KMER_HL = 256;               // histogram bins below this are counted in LDS and added to global memory once per block
constexpr int KMER_ROWS = 16 * 2048;       // DPP rows of a launch at the most (2048 blocks: eight per CU); a row takes items a launch apart

// one level of the enumeration: item i of in[3i ..] = code, lo, hi is an l-mer; its live children are (l+1)-mers.  ctr[0], ctr[1], ctr[2]:
// the cursor of the next segment, the k-mers found, the k-mers that met min_occ before the canonical filter.
//   l + 1 < k   a live child draws a number j from ctr[0] and goes to out[3j ..], the segment of the next level (j < out_cap always holds
//               for the slices the host cuts; a number beyond it is not stored)
//   l + 1 == k  a live child that passes the canonical filter is a k-mer of the result: it draws j from ctr[1], is stored in
//               out[3 * (j - out_base) ..] when j < out_max (max_recs) and the slot lies inside the staging buffer (out_base <= j <
//               out_base + out_cap), and is counted in hist[min(hi - lo, hist_len - 1)]
// One DPP row per item, both ranks by all 16 lanes; lane a - 1 of the row then owns child a.  Numbers are drawn once per wave: a ballot
// of the live children, one atomic by lane 0, the position of a child = the live children in the lanes below it.  Every row of a block
// makes the same number of turns, so the ballots see whole waves.
template <bool SPARSE> __global__ __launch_bounds__(256) void k_kmer_expand(const QTab *Tg, PoolView pv, const int64_t *in, uint64_t n, int l, int k, int64_t min_occ, int canonical,
                                                                            int64_t *out, uint64_t out_cap, uint64_t out_base, uint64_t out_max,
                                                                            unsigned long long *ctr, unsigned long long *hist, int64_t hist_len)
{
	__shared__ QTab T;
	__shared__ uint32_t s_hist[KMER_HL];
	__shared__ uint32_t s_pre;
	static_assert(KMER_HL == 256, "one thread per bin");
	s_hist[threadIdx.x] = 0;
	if (threadIdx.x == 0) s_pre = 0;
	qtab_load(Tg, T);
	const int lane = lane_id();
	const QRow R = qrow();
	const bool last = l + 1 == k;
	for (uint64_t d = 0; R.b + d < n; d += (uint64_t)gridDim.x * QPB) {   // (by the block's first row: the same turns in the whole block)
		const uint64_t i = R.i + d;
		bool live = false;
		uint64_t code = 0, nlo = 0, nhi = 0;
		if (i < n) {
			const uint64_t pc = (uint64_t)in[3 * i], lo = (uint64_t)in[3 * i + 1], hi = (uint64_t)in[3 * i + 2];
			const QPair<SPARSE> P(T, pv, lo, hi);
#pragma unroll
			for (int a = 1; a <= 4; ++a)
				if (R.g == (uint32_t)(a - 1)) P.child(T, a, nlo, nhi);
			code = kmer_prepend(pc, l, (int)R.g + 1);
			live = R.g < 4 && nhi - nlo >= (uint64_t)min_occ;
		}
		if (last) {
			const uint64_t pre = ballot64(live);
			if (lane == 0 && pre) atomicAdd(&s_pre, (uint32_t)__popcll(pre));
			if (canonical) live = live && kmer_canonical(code, k);
		}
		const uint64_t mask = ballot64(live);
		unsigned long long base = 0;
		if (lane == 0 && mask) base = atomicAdd(&ctr[last ? 1 : 0], (unsigned long long)__popcll(mask));
		const uint64_t j = uniform64(base) + (uint64_t)__popcll(mask & lt_mask(lane));
		if (live) {
			if (j < out_max && j >= out_base && j - out_base < out_cap) {
				int64_t *o = out + 3 * (j - out_base);
				o[0] = (int64_t)code; o[1] = (int64_t)nlo; o[2] = (int64_t)nhi;
			}
			if (last && hist_len > 0) {
				const uint64_t bin = min(nhi - nlo, (uint64_t)hist_len - 1);
				if (bin < (uint64_t)KMER_HL) atomicAdd(&s_hist[bin], 1u);
				else atomicAdd(&hist[bin], 1ull);
			}
		}
	}
	if (!last) return;                                              // (the same in the whole block)
	__syncthreads();
	const uint32_t v = s_hist[threadIdx.x];
	if (v) atomicAdd(&hist[threadIdx.x], (unsigned long long)v);     // (a bin that was counted lies below hist_len)
	if (threadIdx.x == 0 && s_pre) atomicAdd(&ctr[2], (unsigned long long)s_pre);
}

// ---- approximate search: the matches of a query within max_mm substitutions ----
// A match of the query q (L symbols) is a word S of L symbols A C G T that differs from q at no more than max_mm positions and has at
// least min_occ occurrences.  Backtracking over the positions L - 1 .. 0: a node is (p, the interval of S[p + 1 ..), the m substitutions so
// far), and one pair of ranks of its interval gives the intervals of its four children, as in k_kmer_expand; the child of q[p] costs
// nothing, the three others one substitution each, an N costs one whatever stands for it.  A child is dropped when its interval is
// smaller than min_occ, or when m + cost + D[p - 1] > max_mm, D being the piece bound of approx_bound (rb2_query_plan.h), which one plain
// backward search over the query computes first.  A live child at position 0 is a match.
//
// One query per DPP row, control uniform within the row; a row takes the queries i = row, row + rows, ... with lmin < L <= lcap (the host
// sorts the lengths into launches that way: stack_passes).  The stack is the path, in the row's part of scr (approx_row_bytes(lrow) bytes):
//   kid[8 p + 2 (a - 1) ..] = lo, hi of child a of the node at position p      (lanes 0 .. 7 store one word each: one 64-byte line)
//   G[p]                      approx_bound's count                             tk[p] = the child taken at p | the next one to try << 3
// so that coming back to a position costs two loads and no rank.  The children are tried in the order q[p], A, C, G, T.  kid is the kid
// line above (kid_store, kid_child) with its two fences.  G and tk are written by every lane with the same value, each lane reads its own.
// Every pair of ranks, those of the bound included, is a step: at max_steps the query ends with cnt = -2 - (matches found so far).  Between
// two steps a row does a bounded amount of other work (four children, and one pop per push), so a launch ends after n * max_steps steps.
// rec[(i * max_recs + k) * 4 ..] = lo, hi, n_mm, subs (approx_push) for k < max_recs, by lanes 0 .. 3; cnt[i] as in include/rb2_hip.h.
template <bool SPARSE> __global__ __launch_bounds__(256) void k_approx(const QTab *Tg, PoolView pv, const uint8_t *qry, const int64_t *off, int64_t base, uint64_t n,
                                                                       int max_mm, int64_t min_occ, int64_t max_steps, int64_t max_recs, int64_t lmin, int64_t lcap,
                                                                       uint64_t rows, int64_t lrow, uint8_t *scr, int64_t *rec, int64_t *cnt)
{
	__shared__ QTab T;
	qtab_load(Tg, T);
	const QRow R = qrow();
	if (R.i >= rows) return;
	const int64_t N = (int64_t)T.row0[NR];
	uint64_t *kid = (uint64_t*)(scr + R.i * (uint64_t)approx_row_bytes(lrow));
	uint8_t *G = (uint8_t*)(kid + 8 * lrow), *tk = G + approx_pad(lrow);
	for (uint64_t i = R.i; i < n; i += rows) {
		const int64_t L = off[i + 1] - off[i];
		if (L <= lmin || L > lcap) continue;                       // another launch takes it
		const QSlice S = qslice<false>(qry, off, base, i, L > min(lrow, APPROX_MAX_LEN));   // (longer than the stack: malformed, and not read)
		if (S.bad || L == 0) { if (R.g == 0) cnt[i] = S.bad ? -1 : 0; continue; }
		int64_t steps = 0, k = 0;
		const int pieces = approx_bound(S.q, L, N, min_occ, max_mm, max_steps, [&](int64_t lo, int64_t hi, int c, int64_t &nlo, int64_t &nhi) {
			QPair<SPARSE>(T, pv, (uint64_t)lo, (uint64_t)hi).child(T, c, nlo, nhi); }, G, &steps);
		if (pieces < 0 || pieces > max_mm) { if (R.g == 0) cnt[i] = pieces < 0 ? -2 : 0; continue; }
		int64_t p = L - 1;
		uint64_t lo = 0, hi = (uint64_t)N, subs = 0;
		int m = 0;
		bool over = false;
		for (;;) {                                                 // the node (p, [lo, hi), m, subs): its children, then the next node in depth-first order
			if (steps >= max_steps) { over = true; break; }
			++steps;
			uint64_t klo[4], khi[4];
			kid_store(T, QPair<SPARSE>(T, pv, lo, hi), kid, p, R.g, klo, khi);
			bool fresh = true, down = false;
			int t = 0;
			for (;;) {                                             // the children of the node at p from try t on; with none left, back to the node behind
				const int c = S.q[p], need = approx_need(G, pieces, p);
				while (t < 5) {
					const int tt = t++, a = tt == 0 ? c : tt, cost = tt != 0;
					if (tt == 0 ? c == 5 : a == c) continue;           // (N has no child of its own; q[p] was try 0)
					if (m + cost + need > max_mm) { if (cost) t = 5; continue; }
					uint64_t xlo = 0, xhi = 0;
					if (fresh) {
#pragma unroll
						for (int b = 0; b < 4; ++b) if (a == b + 1) { xlo = klo[b]; xhi = khi[b]; }
					} else kid_child(kid, p, a, xlo, xhi);
					if ((int64_t)(xhi - xlo) < min_occ) continue;
					if (p == 0) {                                      // a match
						qstore(rec, i, max_recs, k, R.g, xlo, xhi, m + cost, cost ? approx_push(subs, m, 0, a) : subs);
						++k;
						continue;
					}
					if (cost) { subs = approx_push(subs, m, p, a); ++m; }
					tk[p] = (uint8_t)(a | t << 3);
					lo = xlo; hi = xhi; --p; down = true;
					break;
				}
				if (down || ++p == L) break;
				const int b = tk[p];
				t = b >> 3;
				if ((b & 7) != S.q[p]) { subs = approx_pop(subs, m); --m; }
				fresh = false;
				__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
			}
			if (!down) break;                                      // back behind the last position: the search is complete
		}
		if (R.g == 0) cnt[i] = over ? -2 - k : k;
	}
}

// ---- duplicate and contained strings ----
// The walk of string k (row = k, then LF steps to the first `$`) visits the rows of its own suffixes.  Next to the row it carries, for the
// suffix of the j symbols read so far, lo and hi -- [lo, hi) is the interval of that suffix -- and ahi: [lo, ahi) is the interval of the
// suffix followed by `$` (`$` sorts first, so the two share their lower end); all four move to C[c] + occ(c, .) with the symbol c of the
// row, and lo <= row < ahi <= hi holds throughout.  At the `$` the suffix is the whole text S of the string: occ = hi - lo occurrences of S
// in all strings, n_equal = occ($, ahi) - occ($, lo) strings whose text is S, rank = occ($, row) - occ($, lo) of them in front of string k.

// occ(c, x), and *z = occ($, x) if asked: the column of the step out of the six counts of a rank (selects: QPair::at)
template <bool SPARSE> __device__ __forceinline__ uint64_t qocc(const QTab &T, const PoolView &pv, uint64_t x, int c, uint64_t *z = nullptr)
{
	uint64_t v[6];
	qrank<SPARSE>(T, pv, x, v);
	if (z) *z = v[0];
	return QPair<SPARSE>::at(v, c);
}

// rec[5i ..] = flag, occ, n_equal, rank, walked (include/rb2_hip.h) of string ids[i], or of string id0 + i when ids is NULL; one string
// per DPP row.  early: stop with (0, 1, 1, 0, steps) as soon as hi - lo == 1 -- the suffix occurs once, so the string does.  Once
// ahi - lo == 1 the interval [lo, ahi) is the row itself and stays so: ahi is no longer ranked.  The guard is that of k_ssa_build: the
// steps are counted against N and a row is tested against N before it is ranked, so on an index that is no BWT of complete strings a walk
// ends with flag -2 and no row outside the index is read (lo, hi and ahi never exceed N: qrank takes x <= N).
// Left alone the compiler takes 100 VGPRs for the sparse layout (4 waves per SIMD) and 92 for the dense one; held to 5 waves, as k_smem is,
// it needs 91 and 92 and no scratch.
template <bool SPARSE> __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 5))) void k_contain(const QTab *Tg, PoolView pv, const int64_t *ids, int64_t id0, uint64_t n, int early, int64_t *rec)
{
	__shared__ QTab T;
	qtab_load(Tg, T);
	const QRow R = qrow();
	if (R.i >= n) return;
	const uint64_t N = T.row0[NR], nstr = qC(T, 1);
	const int64_t k = ids ? ids[R.i] : id0 + (int64_t)R.i;
	int64_t flag = 0;
	uint64_t occ = 0, neq = 0, rank = 0, j = 0;
	if (k < 0 || (uint64_t)k >= nstr) flag = -1;
	else {
		uint64_t row = (uint64_t)k, lo = 0, hi = N, ahi = nstr;
		for (;;) {
			uint64_t cr[6];
			uint32_t c;
			qrank<SPARSE>(T, pv, row, cr, &c);
			if (c == 0) {                                          // the string's own `$`: [lo, hi) is the interval of its text
				if (j == 0) { flag = 4; break; }
				occ = hi - lo; neq = 1;
				if (ahi - lo != 1) {
					uint64_t zl, zh;
					qocc<SPARSE>(T, pv, lo, 0, &zl); qocc<SPARSE>(T, pv, ahi, 0, &zh);
					neq = zh - zl; rank = cr[0] - zl;
				}
				flag = (rank != 0 ? 1 : 0) | ((int64_t)occ > (int64_t)neq ? 2 : 0);
				break;
			}
			if (j >= N) { flag = -2; break; }
			const uint64_t C = qC(T, (int)c);
			const bool one = ahi - lo == 1;
			row = C + QPair<SPARSE>::at(cr, (int)c);
			lo = C + qocc<SPARSE>(T, pv, lo, (int)c);
			hi = C + qocc<SPARSE>(T, pv, hi, (int)c);
			ahi = one ? min(lo + 1, N) : C + qocc<SPARSE>(T, pv, ahi, (int)c);
			++j;
			if (row >= N) { flag = -2; break; }
			if (early && hi - lo == 1) { occ = neq = 1; break; }
		}
		if (flag < 0 || flag == 4) occ = neq = rank = j = 0;
	}
	qstore(rec, R.i, 1, 0, R.g, flag, occ, neq, rank, j);
}

// ---- irreducible overlaps: the edges of a string graph ----
// The backward search of k_overlap, carrying the bi-interval (x0, x1, sz) as k_smem does: when nd strings begin with the last m symbols
// of the query, [x1, x1 + nd) is the interval of revcomp(those symbols) followed by `$` on an index of both strands (`$` sorts first) --
// an ENTRY (m, lo, hi).  Extending an entry to the left by a is extending the overlap to the right by comp(a), and a `$` in front of it
// (occ($, hi) > occ($, lo)) is a string revcomp(T) that ends there: T = the overlap followed by the extension.  All entries of a query
// are extended together, depth first: a node is the list of entries still alive after d symbols; one pair of ranks per entry gives its
// `$` range and its four children.  The first node of a branch where a string ends is closed with one record -- that of its entry with
// the longest overlap --: what is still alive there is reached through that string.
//
// One query per DPP row, control uniform within the row; a row takes the queries i = row, row + rows, ...  The stack is the path, in the
// row's part of scr (irred_row_bytes(cap, max_ext) bytes), the frames of its nodes behind each other; entry e is written when it is ranked:
//   kid[8 e + 2 (a - 1) ..] = lo, hi of child a of entry e    (lanes 0 .. 7 store one word each: one 64-byte line)      el[e] = its overlap length
//   fs[d], fa[d]              the first entry of frame d and the next child to try there, kept while frame d + 1 is the top one
// so that coming back to a node costs loads and no rank.  kid is the kid line above (kid_store, kid_child) with its fences.  el, fs and fa
// are written by every lane with the same value, each lane reads its own.  The entries of the root are ranked as the search finds them, not behind it: the steps are
// the same, and a query that runs out of them in either has no record yet.
// Every pair of ranks is a step, and every entry written has cost one: at max_steps the query ends with cnt = -2 - (records so far).  The
// frames 0 .. max_ext hold at most L - min_ovlp entries each, so e < cap = irred_entry_cap() whatever the index holds (tested all the same).
// rec[(i * max_recs + k) * 4 ..] = l, ext, zlo, zhi for k < max_recs, by lanes 0 .. 3; cnt[i] as in include/rb2_hip.h.

// ranks the entry (l, [lo, hi)) and writes it as entry e of the stack; zlo, zhi = the `$`s in front of its two ends
template <bool SPARSE> __device__ __forceinline__ void irred_rank(const QTab &T, const PoolView &pv, uint64_t lo, uint64_t hi, uint64_t *kid, uint16_t *el, int64_t e, uint32_t l,
                                                                  uint32_t g, uint64_t &zlo, uint64_t &zhi)
{
	const QPair<SPARSE> P(T, pv, lo, hi);
	uint64_t klo[4], khi[4];
	el[e] = (uint16_t)l;                                       // (in front of the release fence, as the line is)
	kid_store(T, P, kid, e, g, klo, khi);
	zlo = P.cl[0]; zhi = P.ch[0];
}

// END0: every query is followed by one closing 0 inside its slice (the packed strings of rb2_unpack.h, asked as they lie: rb2_graph.h)
template <bool SPARSE, bool END0 = false> __global__ __launch_bounds__(256) void k_irreducible(const QTab *Tg, PoolView pv, const uint8_t *qry, const int64_t *off, int64_t base, uint64_t n,
                                                                            int64_t min_ovlp, int64_t max_ext, int64_t max_steps, int64_t max_recs, int64_t lmax,
                                                                            uint64_t rows, int64_t cap, uint8_t *scr, int64_t *rec, int64_t *cnt)
{
	__shared__ QTab T;
	qtab_load(Tg, T);
	const QRow R = qrow();
	if (R.i >= rows) return;
	const uint64_t N = T.row0[NR];
	const int64_t nf = irred_frames(cap, max_ext);
	uint64_t *kid = (uint64_t*)(scr + R.i * (uint64_t)irred_row_bytes(cap, max_ext));
	uint32_t *fs = (uint32_t*)(kid + 8 * cap);
	uint16_t *el = (uint16_t*)((uint8_t*)fs + irred_pad(4 * nf));
	uint8_t *fa = (uint8_t*)el + irred_pad(2 * cap);
	for (uint64_t i = R.i; i < n; i += rows) {
		const int64_t L = off[i + 1] - off[i] - (END0 ? 1 : 0);
		const QSlice S = qslice<END0>(qry, off, base, i, L > min(lmax, IRRED_MAX_LEN) || (END0 && L < 0));   // (longer than the host sized the stacks for: malformed, and not read)
		if (S.bad || L == 0) { if (R.g == 0) cnt[i] = S.bad ? -1 : 0; continue; }
		int64_t steps = 0, k = 0, top = 0;                         // top: the entries on the stack
		bool over = false;
		const int c0 = S.q[L - 1];
		if (c0 < 5) {                                              // the search: the turn of m ranks the interval of the last m symbols
			uint64_t x0 = qC(T, c0), x1 = qC(T, 5 - c0), sz = qC(T, c0 + 1) - x0;
			for (int64_t m = 1; sz > 0; ++m) {
				if (steps >= max_steps) { over = true; break; }
				++steps;
				const int c = m < L ? S.q[L - 1 - m] : 5;
				uint64_t nd, add, nx0 = 0, nx1 = 0;
				{
					const QPair<SPARSE> P(T, pv, x0, x0 + sz);
					add = nd = P.size(0);                          // the other end in the complement order $ T G C A N
#pragma unroll
					for (int b = 4; b >= 2; --b) if (b > c) add += P.size(b);
					if (c < 5) P.child(T, c, nx0, nx1);
				}
				if (m >= min_ovlp && m < L && nd > 0) {            // an entry of the root
					if (steps >= max_steps || top >= cap) { over = true; break; }
					++steps;
					uint64_t zl, zh;
					irred_rank<SPARSE>(T, pv, min(x1, N), min(x1 + nd, N), kid, el, top, (uint32_t)m, R.g, zl, zh);   // (one strand: the twin interval may leave the index)
					++top;
				}
				if (c == 5) break;                                 // the whole query, or an N
				x1 += add; x0 = nx0; sz = nx1 - nx0;
			}
		}
		if (!over && top > 0) {
			int64_t d = 0, f0 = 0;                                 // the top frame: the node at depth d, entries [f0, top)
			int a = 1;                                             // its next child
			for (;;) {
				if (a > 4) {                                       // no child left: back to the frame below
					if (d == 0) break;
					top = f0; --d;
					f0 = (int64_t)fs[d]; a = fa[d];
					continue;
				}
				int64_t nt = top;                                  // child a, the node at depth d + 1: its entries [top, nt)
				uint32_t bl = 0;
				uint64_t bzl = 0, bzh = 0;
				for (int64_t e = f0; e < top; ++e) {
					__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
					uint64_t lo, hi;
					kid_child(kid, e, a, lo, hi);
					if (lo >= hi) continue;
					if (steps >= max_steps || nt >= cap) { over = true; break; }
					++steps;
					const uint32_t l = el[e];
					uint64_t zl, zh;
					irred_rank<SPARSE>(T, pv, lo, hi, kid, el, nt, l, R.g, zl, zh);
					++nt;
					if (zh > zl && (bzh == bzl || l > bl)) { bl = l; bzl = zl; bzh = zh; }   // a string ends here: the longest overlap names the node
				}
				if (over) break;
				if (bzh > bzl) { qstore(rec, i, max_recs, k, R.g, bl, d + 1, bzl, bzh); ++k; ++a; }
				else if (nt > top && d + 1 < max_ext) { fs[d] = (uint32_t)f0; fa[d] = (uint8_t)(a + 1); ++d; f0 = top; top = nt; a = 1; }
				else ++a;                                          // empty, or as deep as an extension goes
			}
		}
		if (R.g == 0) cnt[i] = over ? -2 - k : k;
	}
}

} // namespace rb2
