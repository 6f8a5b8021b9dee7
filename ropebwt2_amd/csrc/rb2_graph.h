// rb2_graph.h -- the string graph of the index's own strings (the definitions: include/rb2_hip.h, rb2_hip_string_graph).
//
// A chunk of sources is unpacked on the device (rb2_unpack.h), asked with k_irreducible<.., END0> as it lies -- every string followed by its
// closing 0, one offsets array -- and its records become rows src, dst, l, ext in three passes with nothing read back between them:
//   k_graph_cut     one thread, at the head of a chunk: closes the chunk before (the running base of the call moves by its edges) and
//                   cuts the strings tried at the text budget (graph_text_cut); k_graph_lmax: the longest string taken, which sizes the stacks
//   k_graph_count   one thread per source: its edges = the sum over its stored records of min(zhi - zlo, max_hits); the counters of info
//   (scan_launch<ScanSat>, rb2_scan.h: exclusive sums of the counts in place)
//   k_graph_emit    one DPP row (16 lanes) per source: the row walks its records with a running offset, the lanes take the hits of a
//                   record side by side, so the rows of a source are written in their order by neighbouring lanes, 32 bytes each, and
//                   no second scan is needed.  A row at or above cap is not stored; a `$` rank that is no string is not read.
// The words of a call in device memory (gc[]): see the enum.
#pragma once
#include "rb2_unpack.h"
#include "rb2_graph_plan.h"

namespace rb2 {

enum { GR_TOOK = 0, GR_BYTES, GR_LMAX, GR_BASE, GR_OVER_RECS, GR_OVER_HITS, GR_OVER_STEPS, GR_TOO_LONG, GR_CHUNK, GR_WORDS = 16 };

// x[0 .. tried]: the offsets of the strings tried.  gc[GR_TOOK] = the strings of the chunk, gc[GR_BYTES] = their packed text;
// gc[GR_BASE] takes in gc[GR_CHUNK], the edges of the chunk before.  One thread
__global__ void k_graph_cut(const uint64_t *x, uint64_t tried, uint64_t budget, unsigned long long *gc)
{
	if (blockIdx.x != 0 || threadIdx.x != 0) return;
	const uint64_t took = (uint64_t)graph_text_cut(x, (int64_t)tried, budget);
	gc[GR_TOOK] = took; gc[GR_BYTES] = x[took] - x[0]; gc[GR_LMAX] = 0;
	gc[GR_BASE] = ut_sat(gc[GR_BASE], gc[GR_CHUNK]); gc[GR_CHUNK] = 0;
}

// behind it: gc[GR_LMAX] = the longest string the chunk took, with its closing 0 (one atomic per wave)
__global__ __launch_bounds__(256) void k_graph_lmax(const uint64_t *x, unsigned long long *gc)
{
	const uint64_t took = gc[GR_TOOK];
	unsigned long long mx = 0;
	for (uint64_t i = ut_first(); i < took; i += ut_stride()) mx = max(mx, (unsigned long long)(x[i + 1] - x[i]));
	for (int d = 32; d >= 1; d >>= 1) mx = max(mx, (unsigned long long)__shfl_xor(mx, d));
	if (lane_id() == 0 && mx) atomicMax(&gc[GR_LMAX], mx);
}

// the stored records of a source: cnt as rb2_hip_irreducible reports it
__device__ __forceinline__ int64_t graph_have(int64_t c, int64_t max_recs) { return min(budget_found(c), max_recs); }

// the strings of a record's range that become edges
__device__ __forceinline__ uint64_t graph_hits(int64_t zlo, int64_t zhi, int64_t max_hits) { return zhi > zlo ? (uint64_t)min(zhi - zlo, max_hits) : 0; }

// e[i] = the edges of source i of the chunk (n sources, off their n + 1 offsets, rec and cnt as k_irreducible left them)
__global__ __launch_bounds__(256) void k_graph_count(uint64_t n, const int64_t *off, const int64_t *rec, const int64_t *cnt, int64_t max_recs, int64_t max_hits,
                                                     uint64_t *e, unsigned long long *gc)
{
	for (uint64_t i = ut_first(); i < n; i += ut_stride()) {
		const int64_t c = cnt[i], have = graph_have(c, max_recs);
		if (off[i + 1] - off[i] - 1 > IRRED_MAX_LEN) atomicAdd(&gc[GR_TOO_LONG], 1ull);
		if (c <= -2) atomicAdd(&gc[GR_OVER_STEPS], 1ull);
		if (budget_found(c) > max_recs) atomicAdd(&gc[GR_OVER_RECS], 1ull);
		uint64_t sum = 0;
		for (int64_t k = 0; k < have; ++k) {
			const int64_t *r = rec + (i * (uint64_t)max_recs + (uint64_t)k) * 4;
			const int64_t zlo = r[2], zhi = r[3];
			if (zhi > zlo && zhi - zlo > max_hits) atomicAdd(&gc[GR_OVER_HITS], 1ull);
			sum += graph_hits(zlo, zhi, max_hits);
		}
		e[i] = sum;
	}
}

// the rows of the n sources src0 .. src0 + n - 1: row gc[GR_BASE] + e[i] is the first of source i (e: the exclusive sums of the counts)
__global__ __launch_bounds__(256) void k_graph_emit(uint64_t n, int64_t src0, const int64_t *rec, const int64_t *cnt, const uint64_t *e, int64_t max_recs, int64_t max_hits,
                                                    int pairs, const uint64_t *head, uint64_t nstr, const unsigned long long *gc, uint64_t cap, int64_t *edges)
{
	const QRow R = qrow();
	if (R.i >= n) return;
	const int64_t have = graph_have(cnt[R.i], max_recs);
	uint64_t row = ut_sat(gc[GR_BASE], e[R.i]);
	for (int64_t k = 0; k < have && row < cap; ++k) {
		const int64_t *r = rec + (R.i * (uint64_t)max_recs + (uint64_t)k) * 4;
		const int64_t l = r[0], ext = r[1], zlo = r[2], zhi = r[3];
		const uint64_t w = graph_hits(zlo, zhi, max_hits);
		for (uint64_t j = R.g; j < w; j += 16) {
			const uint64_t z = (uint64_t)zlo + j, at = row + j;
			if (at >= cap || zlo < 0 || z >= nstr) continue;
			const int64_t id = (int64_t)head[z];
			int64_t *o = edges + 4 * at;
			o[0] = src0 + (int64_t)R.i; o[1] = pairs ? id ^ 1 : id; o[2] = l; o[3] = ext;
		}
		row += w;
	}
}

} // namespace rb2
