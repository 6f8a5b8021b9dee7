// rb2_unpack.h -- the strings of the index, packed (the definitions: include/rb2_hip.h): a packed inverse BWT.
//
// String k = row k of the `$` block; its walk x_0 = k, x_{j+1} = LF(x_j) reads it last symbol first and ends at the first row whose symbol
// is `$`.  Two passes, one string per DPP row (16 lanes) each:
//   k_unpack_len   walks string first + i and writes len + 1 into x[i] (the symbols and the closing 0); a walk that does not end counts
//                  in *bad.  The guard is k_ssa_build's (ut_walk): steps counted against N, a row tested before it is ranked.
//   (scan_launch<ScanSat>, rb2_scan.h: exclusive sums of x in place -- the offsets)
//   k_unpack_text  walks again and stores.  Lane g of the row keeps the symbol of the steps j with j & 15 == g; behind step 16 q + 15, and
//                  behind the last step, the row stores what it holds with ONE store instruction: lane g writes the byte of step 16 q + g,
//                  sixteen neighbouring bytes of the slice (ascending addresses when reversed, descending in text order: the same packing,
//                  mirrored).  Bytes, one per lane, so an offset of any alignment needs no head and no tail of its own: the last store of
//                  a string is the same instruction with the lanes behind the closing 0 switched off.
// Every store is tested against the slice of its string, [off[i] - base, off[i + 1] - base) inside [0, cap): the walk is cut at the length
// the offsets give, never the other way round, so offsets that belong to another index give wrong bytes inside the slices and nothing else.
#pragma once
#include "rb2_unitig.h"

namespace rb2 {

// x[i] = length of string first + i, plus 1, for the n strings of this launch (x: the offsets-to-be of these strings)
template <bool SPARSE> __global__ __launch_bounds__(256) void k_unpack_len(const QTab *Tg, PoolView pv, uint64_t first, uint64_t n, uint64_t *x, unsigned long long *bad)
{
	__shared__ QTab T;
	qtab_load(Tg, T);
	const QRow R = qrow();
	if (R.i >= n) return;
	const uint64_t k = first + R.i;
	bool ended = false;
	uint64_t len = 0;
	if (k < qC(T, 1)) len = ut_walk<SPARSE>(T, pv, k, ~0ull, &ended, [](uint64_t, uint32_t) {});
	if (R.g != 0) return;
	if (!ended) atomicAdd(bad, 1ull);
	x[R.i] = ended ? len + 1 : 1;
}

// the texts of the n strings from `first` on into txt + off[i] - base; off: their n + 1 offsets
template <bool SPARSE> __global__ __launch_bounds__(256) void k_unpack_text(const QTab *Tg, PoolView pv, uint64_t first, uint64_t n, const int64_t *off, int64_t base, int reversed,
                                                                             int64_t cap, uint8_t *txt)
{
	__shared__ QTab T;
	qtab_load(Tg, T);
	const QRow R = qrow();
	if (R.i >= n) return;
	const int64_t s0 = off[R.i] - base, s1 = off[R.i + 1] - base;          // the slice: len symbols and the closing 0
	if (s0 < 0 || s1 <= s0 || s1 > cap) return;
	const uint64_t N = T.row0[NR], len = min((uint64_t)(s1 - s0 - 1), N);
	uint8_t *o = txt + s0;
	uint64_t x = first + R.i, c6[6];
	uint32_t mine = 0;
	for (uint64_t j = 0; ; ++j) {                                          // step j: symbol len - 1 - j of the string; step len: the closing 0
		const uint32_t c = j < len && x < N ? qlf<SPARSE>(T, pv, x, c6) : 0;
		if ((j & 15) == R.g) mine = c;
		if ((j & 15) == 15 || j == len) {
			const uint64_t jj = (j & ~15ull) + R.g;                        // the step this lane holds
			const int64_t p = jj == len || reversed ? (int64_t)jj : (int64_t)(len - 1 - jj);
			if (jj <= j && p < s1 - s0) o[p] = (uint8_t)mine;
		}
		if (j == len) break;
	}
}

} // namespace rb2
