// rb2_clean.h -- tip and bubble removal on an edge list (the definition: include/rb2_hip.h, rb2_hip_graph_clean).
//
// The caller's rows are never written: a byte per row (dead) says why a row has left -- 0 alive, CL_TIP, CL_BUBBLE --, and an invalid row is
// seen as such from its own words every time.  A round is, one launch each:
//   k_clean_deg     the degrees over the rows alive and, per vertex, (src, ext) of one row into it and dst of one row out of it -- the
//                   first as k_unitig_deg keeps it, for the chain launcher; either is read only where the degree is 1
//   (unitig_rank)   the chains of those rows: vtx = head, rank, off, ext_in per vertex, by the kernels of rb2_unitig.h as they are
//   k_clean_sum     per head: its vertices, the smallest v >> pairs among them, and its tail (the one vertex of an open chain that no
//                   link leaves: a plain store).  The lanes of a wave that name one head add to it once, as in k_unitig_sum
//   k_clean_class   per vertex: the class bits of the chain it heads (0 for every other vertex and for the head of a cycle), and q of an arm
//   k_clean_widen, k_clean_fill   the out-rows of every vertex as a CSR of their dst: the out-degrees as 64-bit words, unitig_scan over
//                   them, and an atomic cursor per vertex; the order inside a vertex is whatever the cursor gives, and nothing sees it
//   k_clean_rival   one thread per arm of at most max_bubble_reads vertices walks the out-rows of its p for an arm of the same q that beats it
//   k_clean_anchor  per row: src has a way out that is no out-tip, dst has a way in that is no in-tip -- bytes, set by plain stores of 1
//   k_clean_mark    per row: removed by a tip rule, else by a bubble rule; the two counts of the round
// and behind the last round k_clean_keep, unitig_scan and k_clean_emit compact the rows kept into out, in input order.
// Every decision reads what the kernels before it wrote and the rows as they were at the start of the round: k_clean_mark is the only
// writer of dead, and nothing in a round reads dead behind it.
#pragma once
#include "rb2_unitig.h"

namespace rb2 {

enum { CL_TIP = 1, CL_BUBBLE = 2 };                             // dead[e]: why row e was removed
enum { CL_OUT_TIP = 1, CL_IN_TIP = 2, CL_ARM = 4, CL_LOSER = 8 };   // cls[h]: the chain h heads
enum { CL_IGNORED = 0, CL_TIPS, CL_BUBBLES, CL_TOTAL, CL_CTRS }; // the counters of a round, in device memory

// per vertex: the degrees and single rows of the round (outdeg, indeg, inedge are the chain launcher's), vtx of its chains, and per head
// cnt = vertices, mn = the smallest v >> pairs, tail, cls, q = dst of the row out of an arm's tail
struct ClV {
	const uint32_t *outdeg, *indeg; const int64_t *inedge; int64_t *outedge; const int64_t *vtx;
	unsigned long long *cnt, *mn; int64_t *tail, *q; uint32_t *cls;
};

__device__ __forceinline__ bool cl_valid(int64_t src, int64_t dst, int64_t ext, uint64_t n) { return src >= 0 && (uint64_t)src < n && dst >= 0 && (uint64_t)dst < n && ext >= 1; }

// the rows alive: degrees and single rows; the invalid rows counted
__global__ __launch_bounds__(256) void k_clean_deg(const int64_t *ed, const uint8_t *dead, uint64_t m, uint64_t n, uint32_t *outdeg, uint32_t *indeg, int64_t *inedge, int64_t *outedge,
                                                   unsigned long long *ctr)
{
	for (uint64_t e = ut_first(); e < m; e += ut_stride()) {
		const int64_t src = ed[4 * e], dst = ed[4 * e + 1], ext = ed[4 * e + 3];
		if (!cl_valid(src, dst, ext, n)) { atomicAdd(&ctr[CL_IGNORED], 1ull); continue; }
		if (dead[e]) continue;
		atomicAdd(&outdeg[src], 1u);
		atomicAdd(&indeg[dst], 1u);
		inedge[2 * dst] = src; inedge[2 * dst + 1] = ext;          // (as k_unitig_deg: nobody reads it where two rows wrote)
		outedge[src] = dst;
	}
}

// per head cnt, mn and tail.  cnt and mn start as 0 and ~0 (the host's memsets); four heads per wave are gathered as in k_unitig_sum
__global__ __launch_bounds__(256) void k_clean_sum(uint64_t n, int pairs, ClV V)
{
	const int lane = lane_id();
	for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x; b < n; b += ut_stride()) {     // (by the block's first vertex: the same turns in the whole block)
		const uint64_t v = b + threadIdx.x;
		const bool live = v < n;
		int64_t h = 0;
		if (live) {
			h = V.vtx[4 * v];
			bool linked = false;                                       // a link leaves v: it is no tail
			if (V.outdeg[v] == 1) linked = V.indeg[V.outedge[v]] == 1;
			if (!linked) V.tail[h] = (int64_t)v;                       // (an open chain has one such vertex; a cycle has none, and its tail is never read)
		}
		uint64_t rest = ballot64(live);
		for (int turn = 0; turn < 4 && rest; ++turn) {
			const int lead = __builtin_ctzll(rest);
			const int64_t h0 = (int64_t)__shfl((unsigned long long)h, lead);
			const uint64_t peers = ballot64(((rest >> lane) & 1) && h == h0);
			if (lane == lead) {                                        // (the lowest lane of its peers: its vertex is their smallest)
				atomicAdd(&V.cnt[h0], (unsigned long long)__popcll(peers));
				atomicMin(&V.mn[h0], (unsigned long long)(v >> pairs));
			}
			rest &= ~peers;
		}
		if ((rest >> lane) & 1) {
			atomicAdd(&V.cnt[h], 1ull);
			atomicMin(&V.mn[h], (unsigned long long)(v >> pairs));
		}
	}
}

// cls[v] and q[v] of every vertex: the class of the open chain v heads
__global__ __launch_bounds__(256) void k_clean_class(uint64_t n, int64_t max_tip, ClV V)
{
	for (uint64_t v = ut_first(); v < n; v += ut_stride()) {
		uint32_t c = 0;
		int64_t q = -1;
		if (V.vtx[4 * v] == (int64_t)v && V.vtx[4 * v + 3] < 1) {      // the head of an open chain
			const int64_t t = V.tail[v];
			const uint32_t in = V.indeg[v], out = V.outdeg[t];
			const bool tiny = V.cnt[v] <= (unsigned long long)max_tip;
			if (tiny && out == 0 && in >= 1) c |= CL_OUT_TIP;
			if (tiny && in == 0 && out >= 1) c |= CL_IN_TIP;
			if (in == 1 && out == 1) {
				q = V.outedge[t];
				if (V.outdeg[V.inedge[2 * v]] >= 2 && V.indeg[q] >= 2) c |= CL_ARM;
			}
		}
		V.cls[v] = c; V.q[v] = q;
	}
}

// x[0 .. n] = the out-degrees and a closing 0: what the scan turns into the first slot of every vertex and the end of the last
__global__ __launch_bounds__(256) void k_clean_widen(uint64_t n, const uint32_t *outdeg, uint64_t *x)
{
	for (uint64_t v = ut_first(); v <= n; v += ut_stride()) x[v] = v < n ? outdeg[v] : 0;
}

// csr[start[src] + its turn] = dst of every row alive; cur[] starts as 0
__global__ __launch_bounds__(256) void k_clean_fill(const int64_t *ed, const uint8_t *dead, uint64_t m, uint64_t n, const uint64_t *start, uint32_t *cur, int64_t *csr)
{
	for (uint64_t e = ut_first(); e < m; e += ut_stride()) {
		const int64_t src = ed[4 * e], dst = ed[4 * e + 1], ext = ed[4 * e + 3];
		if (!cl_valid(src, dst, ext, n) || dead[e]) continue;
		const uint64_t at = start[src] + atomicAdd(&cur[src], 1u);
		if (at < m) csr[at] = dst;                                 // (start and cur come from the same rows: always)
	}
}

// lose[v] = 1 for the head of an arm that loses.  Work: outdeg(p) reads per arm of at most max_bubble vertices
__global__ __launch_bounds__(256) void k_clean_rival(uint64_t n, uint64_t m, int64_t max_bubble, ClV V, const uint64_t *start, const int64_t *csr, uint8_t *lose)
{
	for (uint64_t v = ut_first(); v < n; v += ut_stride()) {
		if (!(V.cls[v] & CL_ARM)) continue;
		const unsigned long long cnt = V.cnt[v], mn = V.mn[v];
		if (cnt > (unsigned long long)max_bubble) continue;
		const int64_t p = V.inedge[2 * v], q = V.q[v];
		bool beaten = false;
		for (uint64_t i = start[p], i1 = min(start[p + 1], m); i < i1 && !beaten; ++i) {
			const int64_t d = csr[i];
			if (d == (int64_t)v || !(V.cls[d] & CL_ARM) || V.q[d] != q) continue;   // (an arm's head has one row into it: the one from p)
			const unsigned long long c2 = V.cnt[d], m2 = V.mn[d];
			beaten = c2 > cnt || (c2 == cnt && m2 < mn);
		}
		if (beaten) lose[v] = 1;
	}
}

// v is the tail of an open chain of class bit: through its head
__device__ __forceinline__ bool cl_tail_of(const ClV &V, int64_t v, uint32_t bit, const uint8_t *lose)
{
	const int64_t h = V.vtx[4 * v];
	if (V.tail[h] != v) return false;
	return bit == CL_LOSER ? lose[h] != 0 : (V.cls[h] & bit) != 0;
}

__global__ __launch_bounds__(256) void k_clean_anchor(const int64_t *ed, const uint8_t *dead, uint64_t m, uint64_t n, ClV V, uint8_t *a_out, uint8_t *a_in)
{
	for (uint64_t e = ut_first(); e < m; e += ut_stride()) {
		const int64_t src = ed[4 * e], dst = ed[4 * e + 1], ext = ed[4 * e + 3];
		if (!cl_valid(src, dst, ext, n) || dead[e]) continue;
		if (!(V.cls[dst] & CL_OUT_TIP)) a_out[src] = 1;
		if (!(V.cls[V.vtx[4 * src]] & CL_IN_TIP) || V.tail[V.vtx[4 * src]] != src) a_in[dst] = 1;
	}
}

// dead[e] of the rows this round removes; their two counts into ctr, once per block.  tips, bubbles: the rule is on
__global__ __launch_bounds__(256) void k_clean_mark(const int64_t *ed, uint8_t *dead, uint64_t m, uint64_t n, ClV V, const uint8_t *a_out, const uint8_t *a_in, const uint8_t *lose,
                                                    int tips, int bubbles, unsigned long long *ctr)
{
	__shared__ unsigned int s_c[2];
	if (threadIdx.x < 2) s_c[threadIdx.x] = 0;
	__syncthreads();
	for (uint64_t e = ut_first(); e < m; e += ut_stride()) {
		const int64_t src = ed[4 * e], dst = ed[4 * e + 1], ext = ed[4 * e + 3];
		if (!cl_valid(src, dst, ext, n) || dead[e]) continue;
		bool tip = false, bub = false;
		if (tips) tip = ((V.cls[dst] & CL_OUT_TIP) && a_out[src]) || (cl_tail_of(V, src, CL_IN_TIP, lose) && a_in[dst]);
		if (!tip && bubbles) bub = lose[dst] || cl_tail_of(V, src, CL_LOSER, lose);   // (lose is set for heads only)
		if (tip) { dead[e] = CL_TIP; atomicAdd(&s_c[0], 1u); }
		else if (bub) { dead[e] = CL_BUBBLE; atomicAdd(&s_c[1], 1u); }
	}
	__syncthreads();
	if (threadIdx.x == 0) {                                        // (a thread makes at most m / 2^24 turns: 32 bits suffice, as in k_unitig_rec)
		if (s_c[0]) atomicAdd(&ctr[CL_TIPS], (unsigned long long)s_c[0]);
		if (s_c[1]) atomicAdd(&ctr[CL_BUBBLES], (unsigned long long)s_c[1]);
	}
}

// x[e] = 1 for a row kept: what the scan numbers
__global__ __launch_bounds__(256) void k_clean_keep(const int64_t *ed, const uint8_t *dead, uint64_t m, uint64_t n, uint64_t *x)
{
	for (uint64_t e = ut_first(); e < m; e += ut_stride()) x[e] = cl_valid(ed[4 * e], ed[4 * e + 1], ed[4 * e + 3], n) && !dead[e] ? 1 : 0;
}

// behind the scan: the rows kept into out, row x[e] below cap
__global__ __launch_bounds__(256) void k_clean_emit(const int64_t *ed, const uint8_t *dead, uint64_t m, uint64_t n, const uint64_t *x, uint64_t cap, int64_t *out)
{
	for (uint64_t e = ut_first(); e < m; e += ut_stride()) {
		const int64_t src = ed[4 * e], dst = ed[4 * e + 1], l = ed[4 * e + 2], ext = ed[4 * e + 3];
		if (!cl_valid(src, dst, ext, n) || dead[e]) continue;
		const uint64_t at = x[e];
		if (at >= cap) continue;
		out[4 * at] = src; out[4 * at + 1] = dst; out[4 * at + 2] = l; out[4 * at + 3] = ext;
	}
}

} // namespace rb2
