// rb2_unitig.h -- the unitigs of a string graph (the definitions: include/rb2_hip.h): the chains of an edge list by
// degree counting and pointer jumping, and their texts out of the index by LF walks that stop early.
//
// Chains (no index is read).  Per vertex four int64, in two buffers A and B that take turns:
//   ptr   a vertex further towards the head of the chain of v (the head itself once the jumps have met it)
//   rank  links between ptr and v          off  the sum of ext over those links          min  the smallest id among the rank vertices
//         behind ptr up to v (v included)
// k_unitig_deg counts the degrees and remembers, per vertex, (src, ext) of one edge into it -- read only where indeg == 1, where that edge
// is the only writer.  k_unitig_link makes the first state: ptr = the predecessor through the link into v, or v itself when there is
// none (and for a self loop: a circular chain of one).  k_unitig_jump reads the state of v and of ptr[v] in one buffer and writes
// (ptr[ptr], rank + rank, off + off, min(min, min)) into the OTHER: the thread of ptr[v] rewrites that vertex's state in the same launch,
// so one buffer would give what the scheduling gives.  After K = ceil(log2(n)) jumps a vertex of an open chain holds its head, rank and off
// (2^K >= n > any rank; a head is a fixed point: (h, 0, 0, h) adds nothing), and a vertex of a cycle holds in min the smallest id of its
// cycle: its 2^K >= n predecessors are all of the cycle, and min does not mind meeting a vertex twice.  k_unitig_cut starts the cycles
// again as paths cut in front of that smallest id (pred[] still holds the first pointers; the vertices of open chains keep their state,
// which further jumps do not change), K more jumps rank them, and k_unitig_fin writes vtx and counts.  The host queues all of this
// without reading anything back: 2 K + 5 launches whatever the graph holds.
//
// Texts.  k_unitig_sum gathers per head (atomics into arrays indexed by the head's id) the vertices, the last off and the smallest id;
// the selected heads are numbered by an exclusive scan over their flags (ScanSat, rb2_scan.h: three launches, saturating sums), their
// lengths come from one walk each (k_unitig_len), the text offsets from a second scan, and then the heads and the other vertices write
// their symbols in launches of their own (k_unitig_text<SPARSE, HEADS>): a head walks a read's length, another vertex ext_in steps.
// Every store is tested against the slice of its chain, and every walk is guarded as k_ssa_build's is, so a vtx that did not come from
// k_unitig_fin, or an edge list of another index, gives wrong bytes inside the slices and nothing else.
#pragma once
#include "rb2_query.h"
#include "rb2_scan.h"

namespace rb2 {

constexpr int UT_BLOCKS = 1 << 16;                 // blocks of a one-thread-per-item launch at the most: the threads stride over the rest
constexpr int UT_ROWS = 16 * 4096;                 // DPP rows of a launch over the selected heads (their number is on the device only)
constexpr uint64_t UT_SAT = SCAN_SAT;              // sums stop here (a text that long is stored nowhere)
constexpr int64_t UT_OFF_MAX = (int64_t)1 << 48;   // an off or ext_in beyond this is no offset into a text: the row is treated as damaged

// the counters of a call, in device memory
enum { UT_IGNORED = 0, UT_CHAINS, UT_CYCLES, UT_LONGEST, UT_NSEL, UT_TOTAL, UT_SHORT, UT_STORED, UT_CTRS };

struct UtState { int64_t ptr, rank, off, min; };

__device__ __forceinline__ uint64_t ut_first() { return (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; }
__device__ __forceinline__ uint64_t ut_stride() { return (uint64_t)gridDim.x * blockDim.x; }
__device__ __forceinline__ uint64_t ut_sat(uint64_t a, uint64_t b) { return ScanSat::op(a, b); }   // (a, b <= UT_SAT)

// edges [e0, e0 + m) of the caller's list, ed = the first of them: one thread per edge
__global__ __launch_bounds__(256) void k_unitig_deg(const int64_t *ed, uint64_t m, uint64_t n, uint32_t *outdeg, uint32_t *indeg, int64_t *inedge, unsigned long long *ctr)
{
	for (uint64_t e = ut_first(); e < m; e += ut_stride()) {
		const int64_t src = ed[4 * e], dst = ed[4 * e + 1], ext = ed[4 * e + 3];
		if (src < 0 || (uint64_t)src >= n || dst < 0 || (uint64_t)dst >= n || ext < 1) { atomicAdd(&ctr[UT_IGNORED], 1ull); continue; }
		atomicAdd(&outdeg[src], 1u);
		atomicAdd(&indeg[dst], 1u);
		inedge[2 * dst] = src; inedge[2 * dst + 1] = ext;          // (two edges into dst: either, or a mixture; nobody reads it then)
	}
}

// the first state (into st) and pred[], ext_in (vtx[4v + 3])
__global__ __launch_bounds__(256) void k_unitig_link(uint64_t n, const uint32_t *outdeg, const uint32_t *indeg, const int64_t *inedge, UtState *st, int64_t *pred, int64_t *vtx)
{
	for (uint64_t v = ut_first(); v < n; v += ut_stride()) {
		int64_t p = (int64_t)v, ext = -1;
		if (indeg[v] == 1) {
			const int64_t u = inedge[2 * v];
			if (outdeg[u] == 1) { p = u; ext = inedge[2 * v + 1]; }
		}
		const bool linked = p != (int64_t)v;
		st[v] = {p, linked ? 1 : 0, linked ? ext : 0, (int64_t)v};
		pred[v] = p;
		vtx[4 * v + 3] = ext;                                      // (a self loop: p == v and ext >= 1, the closing link of a cycle of one)
	}
}

// one doubling, from in to out (never the same buffer)
__global__ __launch_bounds__(256) void k_unitig_jump(uint64_t n, const UtState *in, UtState *out)
{
	for (uint64_t v = ut_first(); v < n; v += ut_stride()) {
		const UtState s = in[v], t = in[s.ptr];
		out[v] = {t.ptr, (int64_t)((uint64_t)s.rank + (uint64_t)t.rank), (int64_t)((uint64_t)s.off + (uint64_t)t.off), min(s.min, t.min)};
	}
}

// behind the first K jumps: a vertex whose ptr was no head at the start lies on a cycle; the cycle starts again as a path from its smallest id
__global__ __launch_bounds__(256) void k_unitig_cut(uint64_t n, const UtState *in, UtState *out, const int64_t *pred, const int64_t *vtx)
{
	for (uint64_t v = ut_first(); v < n; v += ut_stride()) {
		UtState s = in[v];
		if (pred[s.ptr] != s.ptr) {
			if (s.min == (int64_t)v) s = {(int64_t)v, 0, 0, (int64_t)v};
			else s = {pred[v], 1, vtx[4 * v + 3], (int64_t)v};
		}
		out[v] = s;
	}
}

// vtx[4v ..] = head, rank, off (ext_in is there already); chains, cycles and the longest chain into ctr, once per block
__global__ __launch_bounds__(256) void k_unitig_fin(uint64_t n, const UtState *st, int64_t *vtx, unsigned long long *ctr)
{
	__shared__ unsigned long long s_c[3];
	if (threadIdx.x < 3) s_c[threadIdx.x] = 0;
	__syncthreads();
	for (uint64_t v = ut_first(); v < n; v += ut_stride()) {
		const UtState s = st[v];
		vtx[4 * v] = s.ptr; vtx[4 * v + 1] = s.rank; vtx[4 * v + 2] = s.off;
		if (s.ptr == (int64_t)v) { atomicAdd(&s_c[0], 1ull); if (vtx[4 * v + 3] >= 1) atomicAdd(&s_c[1], 1ull); }
		atomicMax(&s_c[2], (unsigned long long)s.rank + 1);
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		if (s_c[0]) atomicAdd(&ctr[UT_CHAINS], s_c[0]);
		if (s_c[1]) atomicAdd(&ctr[UT_CYCLES], s_c[1]);
		atomicMax(&ctr[UT_LONGEST], s_c[2]);
	}
}

// info[0 .. 4) of rb2_hip_unitig_chains_dev out of the counters
__global__ void k_unitig_info(const unsigned long long *ctr, int64_t *info)
{
	if (threadIdx.x == 0 && blockIdx.x == 0) { info[0] = (int64_t)ctr[UT_CHAINS]; info[1] = (int64_t)ctr[UT_CYCLES]; info[2] = (int64_t)ctr[UT_LONGEST]; info[3] = (int64_t)ctr[UT_IGNORED]; }
}

// ---- texts ----

// per head, indexed by its id: cnt = vertices, off = the last off, mn = the smallest id, flg = bit 0 circular | bit 1 a short piece,
// u = its number among the selected chains (-1: not selected)
struct UtHeads { unsigned long long *cnt, *off, *mn; uint32_t *flg; int64_t *u; };
// per selected chain u: head, len = the length of the head's text, tlen = of the chain's, toff = its text offset
struct UtSel { int64_t *head; uint64_t *len, *tlen, *toff; };

// the head a row of vtx names: its own vertex when the row names none (damaged: the vertex is a chain of its own)
__device__ __forceinline__ int64_t ut_head(const int64_t *vtx, uint64_t v, uint64_t n, bool *damaged)
{
	const int64_t h = vtx[4 * v];
	*damaged = h < 0 || (uint64_t)h >= n;
	return *damaged ? (int64_t)v : h;
}

// The vertices of a wave that name one head add to it once: atomics on one word are served one after the other (12 ns each), and one
// chain of a million vertices is otherwise a million of them on each of three words.  Four heads per wave are gathered that way -- the
// two strands of one long unitig alternate from lane to lane --, what is left adds for itself.
__global__ __launch_bounds__(256) void k_unitig_sum(uint64_t n, const int64_t *vtx, UtHeads H)
{
	const int lane = lane_id();
	for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x; b < n; b += ut_stride()) {     // (by the block's first vertex: the same turns in the whole block)
		const uint64_t v = b + threadIdx.x;
		const bool live = v < n;
		int64_t h = 0;
		unsigned long long last = 0;                               // the off this vertex adds (0: none)
		uint32_t f = 0;
		if (live) {
			bool damaged;
			h = ut_head(vtx, v, n, &damaged);
			const int64_t off = vtx[4 * v + 2], ext = vtx[4 * v + 3];
			if (damaged) f = 2u;
			if (h == (int64_t)v) { if (!damaged && ext >= 1) f |= 1u; }
			else if (off < 0 || off > UT_OFF_MAX || ext < 0 || ext > UT_OFF_MAX) f |= 2u;   // no piece of a text: it adds nothing
			else last = (unsigned long long)off;
		}
		uint64_t rest = ballot64(live);                            // the lanes that have not added yet (the same value in the whole wave)
		for (int turn = 0; turn < 4 && rest; ++turn) {
			const int lead = __builtin_ctzll(rest);
			const int64_t h0 = (int64_t)__shfl((unsigned long long)h, lead);
			const uint64_t peers = ballot64(((rest >> lane) & 1) && h == h0);
			const bool mine = (peers >> lane) & 1;
			unsigned long long mx = mine ? last : 0;
			uint32_t fo = mine ? f : 0;
			for (int d = 32; d; d >>= 1) { mx = max(mx, (unsigned long long)__shfl_xor(mx, d)); fo |= (uint32_t)__shfl_xor((int)fo, d); }
			if (lane == lead) {                                    // (the lowest lane of its peers: its vertex is their smallest)
				atomicAdd(&H.cnt[h0], (unsigned long long)__popcll(peers));
				atomicMin(&H.mn[h0], (unsigned long long)v);
				if (mx) atomicMax(&H.off[h0], mx);
				if (fo) atomicOr(&H.flg[h0], fo);
			}
			rest &= ~peers;
		}
		if ((rest >> lane) & 1) {
			atomicAdd(&H.cnt[h], 1ull);
			atomicMin(&H.mn[h], (unsigned long long)v);
			if (last) atomicMax(&H.off[h], last);
			if (f) atomicOr(&H.flg[h], f);
		}
	}
}

__device__ __forceinline__ bool ut_selected(const UtHeads &H, uint64_t h, int canonical, int64_t min_reads)
{
	return H.cnt[h] >= (unsigned long long)min_reads && !(canonical && (H.mn[h] & 1));
}

// u[h] = 1 for a selected head, 0 otherwise: what the scan numbers
__global__ __launch_bounds__(256) void k_unitig_sel(uint64_t n, UtHeads H, int canonical, int64_t min_reads)
{
	for (uint64_t h = ut_first(); h < n; h += ut_stride()) H.u[h] = ut_selected(H, h, canonical, min_reads) ? 1 : 0;
}

// behind the first scan: the selected heads in their order, u[h] = -1 for the others
__global__ __launch_bounds__(256) void k_unitig_list(uint64_t n, UtHeads H, UtSel S, int canonical, int64_t min_reads)
{
	for (uint64_t h = ut_first(); h < n; h += ut_stride()) {
		if (ut_selected(H, h, canonical, min_reads)) S.head[H.u[h]] = (int64_t)h;
		else H.u[h] = -1;
	}
}

// the walk of string k from its row to its `$`, at most lim steps: f(step, symbol) for every symbol, last symbol first.  Returns the
// steps taken, *ended = the `$` was met.  The guard of k_ssa_build: steps counted against N, a row tested before it is ranked.
template <bool SPARSE, typename F> __device__ __forceinline__ uint64_t ut_walk(const QTab &T, const PoolView &pv, uint64_t k, uint64_t lim, bool *ended, F f)
{
	const uint64_t N = T.row0[NR];
	uint64_t x = k, j = 0, c6[6];
	*ended = false;
	while (j < lim && j < N && x < N) {
		const uint32_t c = qlf<SPARSE>(T, pv, x, c6);
		if (c == 0) { *ended = true; break; }
		f(j, c);
		++j;
	}
	return j;
}

// the lengths: one selected head per DPP row, the rows stride over the nsel (= ctr[UT_NSEL]) of them
template <bool SPARSE> __global__ __launch_bounds__(256) void k_unitig_len(const QTab *Tg, PoolView pv, uint64_t n, const unsigned long long *ctr, UtHeads H, UtSel S)
{
	__shared__ QTab T;
	qtab_load(Tg, T);
	const QRow R = qrow();
	const uint64_t nsel = min((uint64_t)ctr[UT_NSEL], n), nstr = qC(T, 1);
	for (uint64_t u = R.i; u < nsel; u += (uint64_t)gridDim.x * QPB) {
		const uint64_t h = (uint64_t)S.head[u];
		bool ended = false;
		uint64_t len = 0;
		if (h < nstr) len = ut_walk<SPARSE>(T, pv, h, ~0ull, &ended, [](uint64_t, uint32_t) {});
		if (!ended) { len = 0; if (R.g == 0) atomicOr(&H.flg[h], 2u); }      // no string of this index: no text
		if (R.g == 0) { S.len[u] = len; S.tlen[u] = len + H.off[h]; S.toff[u] = len + H.off[h]; }   // (toff: what the second scan sums in place)
	}
}

__device__ __forceinline__ bool ut_stored(const UtSel &S, uint64_t u, int64_t cap_u, int64_t cap_txt)
{
	return u < (uint64_t)cap_u && S.toff[u] <= (uint64_t)cap_txt && S.tlen[u] <= (uint64_t)cap_txt - S.toff[u];
}

// HEADS: one selected chain per DPP row (strided as in k_unitig_len); a stored one writes the text of its head into the front of its slice.
// !HEADS: one vertex per DPP row, v = v0 + its number; a vertex that is no head walks ext_in steps -- step k is the symbol at
// len(head) + off(v) - 1 - k of its chain -- and stores them when the chain is stored; a `$` before that is a short piece: zeros in front.
template <bool SPARSE, bool HEADS> __global__ __launch_bounds__(256) void k_unitig_text(const QTab *Tg, PoolView pv, uint64_t n, uint64_t v0, uint64_t nv, const int64_t *vtx,
                                                                                         const unsigned long long *ctr, UtHeads H, UtSel S, int64_t cap_u, int64_t cap_txt, uint8_t *txt)
{
	__shared__ QTab T;
	qtab_load(Tg, T);
	const QRow R = qrow();
	const uint64_t nstr = qC(T, 1);
	if (HEADS) {
		const uint64_t nsel = min((uint64_t)ctr[UT_NSEL], n);
		for (uint64_t u = R.i; u < nsel; u += (uint64_t)gridDim.x * QPB) {
			if (!ut_stored(S, u, cap_u, cap_txt)) continue;
			const uint64_t len = S.len[u];
			uint8_t *o = txt + S.toff[u];
			bool ended;
			ut_walk<SPARSE>(T, pv, (uint64_t)S.head[u], len, &ended, [&](uint64_t k, uint32_t c) { if (R.g == 0) o[len - 1 - k] = (uint8_t)c; });   // (k < len <= tlen)
		}
		return;
	}
	if (R.i >= nv) return;
	const uint64_t v = v0 + R.i;
	bool damaged;
	const int64_t h = ut_head(vtx, v, n, &damaged), off = vtx[4 * v + 2], ext = vtx[4 * v + 3];
	if (h == (int64_t)v || off < 0 || off > UT_OFF_MAX || ext < 0 || ext > UT_OFF_MAX) return;
	const int64_t u = H.u[h];
	if (u < 0) return;
	const bool st = ut_stored(S, (uint64_t)u, cap_u, cap_txt);
	const int64_t tlen = (int64_t)min(S.tlen[u], UT_SAT), end = (int64_t)min(S.len[u], UT_SAT) + off;   // the piece is [end - ext, end) of the chain's text
	uint8_t *o = txt + S.toff[u];
	bool ended = false;
	uint64_t got = 0;
	if (v < nstr) got = ut_walk<SPARSE>(T, pv, v, (uint64_t)ext, &ended, [&](uint64_t k, uint32_t c) {
		const int64_t p = end - 1 - (int64_t)k;
		if (st && R.g == 0 && p >= 0 && p < tlen) o[p] = (uint8_t)c; });
	if (got == (uint64_t)ext) return;
	if (R.g == 0) atomicOr(&H.flg[h], 2u);                         // shorter than its ext_in: zeros in front of what there was, inside the slice
	if (!st) return;
	const int64_t lo = max(end - ext, (int64_t)0), hi = min(end - (int64_t)got, tlen);
	for (int64_t p = lo + R.g; p < hi; p += 16) o[p] = 0;
}

// urec[5u ..] = head, n_reads, text_off, text_len, flags of the stored chains; the chains with a short piece and the stored ones into ctr
__global__ __launch_bounds__(256) void k_unitig_rec(uint64_t n, unsigned long long *ctr, UtHeads H, UtSel S, int64_t cap_u, int64_t cap_txt, int64_t *urec)
{
	__shared__ unsigned int s_c[2];
	if (threadIdx.x < 2) s_c[threadIdx.x] = 0;
	__syncthreads();
	const uint64_t nsel = min((uint64_t)ctr[UT_NSEL], n);
	for (uint64_t u = ut_first(); u < nsel; u += ut_stride()) {
		const int64_t h = S.head[u];
		const uint32_t f = H.flg[h];
		if (f & 2u) atomicAdd(&s_c[0], 1u);
		if (!ut_stored(S, u, cap_u, cap_txt)) continue;
		atomicAdd(&s_c[1], 1u);
		int64_t *r = urec + 5 * u;
		r[0] = h; r[1] = (int64_t)H.cnt[h]; r[2] = (int64_t)S.toff[u]; r[3] = (int64_t)S.tlen[u]; r[4] = (int64_t)f;
	}
	__syncthreads();
	if (threadIdx.x == 0) {                                        // (a thread makes at most n / 2^24 turns: the 32 bits of a block's count suffice up to 2^36 vertices)
		if (s_c[0]) atomicAdd(&ctr[UT_SHORT], (unsigned long long)s_c[0]);
		if (s_c[1]) atomicAdd(&ctr[UT_STORED], (unsigned long long)s_c[1]);
	}
}

} // namespace rb2
