// rb2_correct.h -- reads corrected by the k-mer spectrum of the index (the rule: include/rb2_hip.h and
// correct_read in rb2_correct_plan.h, which this kernel and tests/correct_plan_check.cpp both compile).
//
// One read per DPP row of 16 lanes, control uniform within the row; a row takes the reads row, row + rows, ...  The row first copies its
// read into the output (lane g the bytes g, g + 16, ...: whole 16-byte pieces) and tests the codes on the way; from then on the read
// lives in the output text, where a fix is one byte stored by every lane of the row with the same value, so that each lane reads back
// its own store.  The copy is read by other lanes than wrote it: the vector memory operations of one wave are performed in order, the
// fences keep the compiler from moving them (k_approx).
// The solid bits, one per window, are 1 KiB of LDS per row (CORRECT_MAX_LEN bits): written by every lane of the row with the same value.
// A probe is a backward search over the k symbols of a window, from the interval of its last symbol (no rank) down to its first or to an
// empty interval: at most k - 1 pairs of ranks, so a launch ends after n * max_probes * k pairs whatever the index holds.
#pragma once
#include "rb2_query.h"
#include "rb2_correct_plan.h"

namespace rb2 {

struct CorrectText {
	uint8_t *o;
	__device__ __forceinline__ int get(int64_t x) const { return o[x]; }
	__device__ __forceinline__ void set(int64_t p, int b)
	{
		o[p] = (uint8_t)b;
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
	}
};

struct CorrectBits {
	uint32_t *w;
	__device__ __forceinline__ bool get(int64_t j) const { return w[j >> 5] >> (j & 31) & 1u; }
	__device__ __forceinline__ void set(int64_t j, bool v) { const uint32_t m = 1u << (j & 31), x = w[j >> 5]; w[j >> 5] = v ? x | m : x & ~m; }
};

// item it of the launch is string it * stride of the packed batch: q = qry[off[s] - base, off[s + 1] - base) (END0: the last byte of the
// slice is the closing 0 of a packed string and no symbol of the read), answered in out at the same place; cnt[it], weak[it] as in
// include/rb2_hip.h.  out == qry is allowed: the copy then stores what it loaded.
template <bool SPARSE, bool END0 = false> __global__ __launch_bounds__(256) void k_correct(const QTab *Tg, PoolView pv, const uint8_t *qry, const int64_t *off, int64_t base, uint64_t n,
                                                                                        uint64_t stride, int64_t k, int64_t min_occ, int64_t max_fix, int64_t max_probes, uint64_t rows,
                                                                                        uint8_t *out, int64_t *cnt, int64_t *weak)
{
	__shared__ QTab T;
	__shared__ uint32_t s_solid[QPB][CORRECT_SOLID_WORDS];
	qtab_load(Tg, T);
	const QRow R = qrow();
	if (R.i >= rows) return;
	CorrectBits solid = {s_solid[threadIdx.x >> 4]};
	for (uint64_t it = R.i; it < n; it += rows) {
		const uint64_t s = it * stride;
		const int64_t s0 = off[s] - base, len = off[s + 1] - base - s0, L = len - (END0 ? 1 : 0);
		bool bad = s0 < 0 || L < 0;
		uint8_t *o = out + s0;
		if (!bad) {
			uint32_t nb = 0;
			for (int64_t x = R.g; x < len; x += 16) {
				const uint8_t c = qry[s0 + x];
				o[x] = c;
				nb |= x < L ? (uint32_t)(c < 1 || c > 5) : (uint32_t)(c != 0);
			}
			bad = row_sum16(nb) != 0 || L > CORRECT_MAX_LEN;
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
			__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
		}
		CorrectOut res = {-1, -1};
		if (!bad) {
			CorrectText txt = {o};
			res = correct_read(txt, solid, L, k, min_occ, max_fix, max_probes, [&](int64_t j, int64_t p, int b) -> int64_t {
				int c = p == j + k - 1 ? b : (int)o[j + k - 1];
				uint64_t lo = qC(T, c), hi = qC(T, c + 1);
				for (int64_t x = j + k - 2; x >= j && lo < hi; --x) {
					c = x == p ? b : (int)o[x];
					const QPair<SPARSE> P(T, pv, lo, hi);
					P.child(T, c, lo, hi);
				}
				return hi > lo ? (int64_t)(hi - lo) : 0; });
		}
		if (R.g == 0) { cnt[it] = res.cnt; weak[it] = res.weak; }
	}
}

// ---- rb2_hip_correct_into: from the corrected text of a batch to an insert batch ----
// a = the batch as it was unpacked (text order, every string closed by a 0), b = the same batch as k_correct<., true> left it (the strings
// it * stride corrected, the others not written).  ctr: CORRECT_CTRS counters of the whole call.

enum { CC_CHANGED = 0, CC_FIXES, CC_WEAK, CC_OVER, CC_BAD, CORRECT_CTRS = 8 };

// item it: counts string s = it * stride (changed = its text in b differs from a) and, with stride == 2, writes its mate s + 1 into b as an
// insert batch takes it, last symbol first: the reverse complement of the corrected string read backwards is its complement read forwards.
// A mate of another length than its read (the caller promised otherwise) keeps its own symbols where the read has none.
__global__ __launch_bounds__(256) void k_correct_mate(uint64_t n, uint64_t stride, const uint8_t *a, uint8_t *b, const int64_t *off, int64_t base, const int64_t *cnt, const int64_t *weak,
                                                      unsigned long long *ctr)
{
	const QRow R = qrow();
	if (R.i >= n) return;
	const uint64_t s = R.i * stride;
	const int64_t s0 = off[s] - base, L = off[s + 1] - base - s0 - 1;
	uint32_t diff = 0;
	for (int64_t x = R.g; x < L; x += 16) diff |= (uint32_t)(a[s0 + x] != b[s0 + x]);
	diff = row_sum16(diff);
	if (R.g == 0) {
		const int64_t c = cnt[R.i], f = budget_found(c);
		if (diff) atomicAdd(&ctr[CC_CHANGED], 1ull);
		if (f) atomicAdd(&ctr[CC_FIXES], (unsigned long long)f);
		if (weak[R.i] > 0) atomicAdd(&ctr[CC_WEAK], 1ull);
		if (c <= -2) atomicAdd(&ctr[CC_OVER], 1ull);
		if (c == -1) atomicAdd(&ctr[CC_BAD], 1ull);
	}
	if (stride != 2) return;
	const int64_t m0 = off[s + 1] - base, M = off[s + 2] - base - m0 - 1;
	for (int64_t x = R.g; x <= M; x += 16) {
		const uint8_t c = x == M ? 0 : x < L ? b[s0 + x] : a[m0 + M - 1 - x];
		b[m0 + x] = x < L && x < M && c >= 1 && c <= 4 ? (uint8_t)(5 - c) : c;
	}
}

// item it: string it * stride of b turned round in place (its closing 0 stays); lane g swaps the symbols x and L - 1 - x for x = g, g + 16, ...
__global__ __launch_bounds__(256) void k_correct_reverse(uint64_t n, uint64_t stride, uint8_t *b, const int64_t *off, int64_t base)
{
	const QRow R = qrow();
	if (R.i >= n) return;
	const uint64_t s = R.i * stride;
	const int64_t s0 = off[s] - base, L = off[s + 1] - base - s0 - 1;
	for (int64_t x = R.g; 2 * x + 1 < L; x += 16) {
		const uint8_t u = b[s0 + x], v = b[s0 + L - 1 - x];
		b[s0 + x] = v; b[s0 + L - 1 - x] = u;
	}
}

} // namespace rb2
