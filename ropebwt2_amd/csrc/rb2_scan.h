// rb2_scan.h -- the prefix scans outside the round path: one block-level scan, one scan by a single block (a loop over it) and one scan
// over many blocks in three launches.  The rounds keep their own (block_excl_add and the k_tscan* / k_sbscan* kernels: rb2_device.h,
// rb2_kernels.h).  tests/test_scan_gpu.py runs every form below through rb2_hip_scan_check.
//
// An operation is a struct Op: type, ident(), in(v) (what an input counts as), op(a, b) (associative; a in front of b) and inclusive
// (whether item i of the result holds the items up to and including i, or the items in front of it).
// An input is a functor In: n() on the device (the host may know an upper bound only) and operator()(i) for i < n().
#pragma once
#include "rb2_device.h"

namespace rb2 {

constexpr int SCAN_PER = 4;                        // items per thread of the three-launch scan, side by side: few, so that a load of a wave stays
                                                   // within a few lines (at 16 the .fmd encoder's sizing pass took 60 % longer)
constexpr int SCAN_ITEMS = 256 * SCAN_PER;         // ... and per block
constexpr uint64_t SCAN_SAT = 1ull << 62;          // where ScanSat stops

template <typename T> struct ScanAdd {             // out[i] = the sum of the items in front of i (wraps as T does)
	using type = T;
	static constexpr bool inclusive = false;
	static __device__ __forceinline__ T ident() { return 0; }
	static __device__ __forceinline__ T in(T v) { return v; }
	static __device__ __forceinline__ T op(T a, T b) { return a + b; }
};
struct ScanSat {                                   // the same, and a sum stops at SCAN_SAT; an item counts as SCAN_SAT at the most
	using type = uint64_t;
	static constexpr bool inclusive = false;
	static __device__ __forceinline__ uint64_t ident() { return 0; }
	static __device__ __forceinline__ uint64_t in(uint64_t v) { return min(v, SCAN_SAT); }
	static __device__ __forceinline__ uint64_t op(uint64_t a, uint64_t b) { return min(a + b, SCAN_SAT); }   // (a, b <= SCAN_SAT)
};
struct ScanMax {                                   // out[i] = the largest item up to and including i
	using type = uint64_t;
	static constexpr bool inclusive = true;
	static __device__ __forceinline__ uint64_t ident() { return 0; }
	static __device__ __forceinline__ uint64_t in(uint64_t v) { return v; }
	static __device__ __forceinline__ uint64_t op(uint64_t a, uint64_t b) { return max(a, b); }
};
template <typename T> struct ScanIn {              // an array of n items, n known to the host
	const T *v; uint64_t nn;
	__device__ __forceinline__ uint64_t n() const { return nn; }
	__device__ __forceinline__ T operator()(uint64_t i) const { return v[i]; }
};

// what the threads in front of this one hold together (ident() for the first); *total = the whole block's.  s_w: blockDim.x / 64 words
template <class Op> __device__ __forceinline__ typename Op::type block_excl(typename Op::type v, typename Op::type *s_w, typename Op::type *total)
{
	using T = typename Op::type;
	const int l = lane_id(), w = wave_id(), nw = blockDim.x >> 6;
	T inc = v;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) { const T t = __shfl_up(inc, d); if (l >= d) inc = Op::op(t, inc); }
	if (l == 63) s_w[w] = inc;
	__syncthreads();
	T off = Op::ident(), tot = Op::ident();
	for (int i = 0; i < nw; ++i) { const T x = s_w[i]; if (i < w) off = Op::op(off, x); tot = Op::op(tot, x); }
	__syncthreads();
	*total = tot;
	const T prev = __shfl_up(inc, 1);                              // the lane in front, inclusive; lane 0 has the waves in front alone
	return l ? Op::op(off, prev) : off;
}

// ---- by one block: out[first + i] for i < n from in(first + i), every thread of the block in every turn; run = what lies in front, and
// behind the call run holds these items as well.  out may be the array in reads (a turn loads its items before it stores any) ----
template <class Op, bool INCL = Op::inclusive, class In> __device__ __forceinline__ void scan_by_block(const In &in, typename Op::type *out, uint64_t first, uint64_t n, typename Op::type &run, typename Op::type *s_w)
{
	using T = typename Op::type;
	for (uint64_t i0 = 0; i0 < n; i0 += blockDim.x) {
		const uint64_t i = i0 + threadIdx.x;
		const T v = i < n ? Op::in((T)in(first + i)) : Op::ident();
		T tot;
		const T ex = block_excl<Op>(v, s_w, &tot);
		if (i < n) out[first + i] = Op::op(run, INCL ? Op::op(ex, v) : ex);
		run = Op::op(run, tot);
	}
}
// one block of THREADS: out[0 .. n) and out[n] = the total
template <class Op, class In, int THREADS> __global__ __launch_bounds__(THREADS) void k_scan_block(In in, typename Op::type *out)
{
	__shared__ typename Op::type s_w[THREADS / 64];
	const uint64_t n = in.n();
	typename Op::type run = Op::ident();
	scan_by_block<Op>(in, out, 0, n, run, s_w);
	if (threadIdx.x == 0) out[n] = run;
}

// ---- by many blocks of 256, SCAN_ITEMS items each, in three launches: part[b] = the items of block b; part[b] = the items in front of
// block b (one block; exclusive whatever Op::inclusive says), *total = all; the items again behind their block's part.  The grids are
// sized from the host's upper bound of n(); a block behind n() does nothing ----
template <class Op, class In> __global__ __launch_bounds__(256) void k_scan_part(In in, typename Op::type *part)
{
	using T = typename Op::type;
	__shared__ T s_w[4];
	const uint64_t n = in.n(), i0 = (uint64_t)blockIdx.x * SCAN_ITEMS + (uint64_t)threadIdx.x * SCAN_PER;
	if ((uint64_t)blockIdx.x * SCAN_ITEMS >= n) return;
	T v = Op::ident(), tot;
#pragma unroll
	for (int k = 0; k < SCAN_PER; ++k) if (i0 + k < n) v = Op::op(v, Op::in((T)in(i0 + k)));
	block_excl<Op>(v, s_w, &tot);
	if (threadIdx.x == 0) part[blockIdx.x] = tot;
}
template <class Op, class In> __global__ __launch_bounds__(256) void k_scan_top(In in, typename Op::type *part, typename Op::type *total)
{
	using T = typename Op::type;
	__shared__ T s_w[4];
	T run = Op::ident();
	scan_by_block<Op, false>(ScanIn<T>{part, 0}, part, 0, (in.n() + SCAN_ITEMS - 1) / SCAN_ITEMS, run, s_w);
	if (threadIdx.x == 0 && total) *total = run;
}
// out == the array in reads is allowed: a block loads all its items before it stores the first.  tail: out[n] = the total as well
template <class Op, class In> __global__ __launch_bounds__(256) void k_scan_apply(In in, const typename Op::type *part, typename Op::type *out, int tail)
{
	using T = typename Op::type;
	__shared__ T s_w[4];
	const uint64_t n = in.n(), i0 = (uint64_t)blockIdx.x * SCAN_ITEMS + (uint64_t)threadIdx.x * SCAN_PER;
	if (tail && n == 0 && blockIdx.x == 0 && threadIdx.x == 0) out[0] = Op::ident();
	if ((uint64_t)blockIdx.x * SCAN_ITEMS >= n) return;
	T a[SCAN_PER], v = Op::ident(), tot;
#pragma unroll
	for (int k = 0; k < SCAN_PER; ++k) { a[k] = i0 + k < n ? Op::in((T)in(i0 + k)) : Op::ident(); v = Op::op(v, a[k]); }
	T run = Op::op(part[blockIdx.x], block_excl<Op>(v, s_w, &tot));   // (two barriers: every load of the block lies in front of them)
#pragma unroll
	for (int k = 0; k < SCAN_PER; ++k) {
		if (i0 + k >= n) break;
		if (!Op::inclusive) out[i0 + k] = run;
		run = Op::op(run, a[k]);
		if (Op::inclusive) out[i0 + k] = run;
		if (tail && i0 + k + 1 == n) out[n] = run;
	}
}

// words of part[] that a scan of up to n items needs
inline size_t scan_parts(uint64_t n) { return (size_t)((n + SCAN_ITEMS - 1) / SCAN_ITEMS) + 1; }

// the three launches on st: in.n() <= n_ub items, part = scan_parts(n_ub) words; total (or NULL) gets the total, and out[n] with tail
template <class Op, class In> void scan_launch(hipStream_t st, In in, uint64_t n_ub, typename Op::type *part, typename Op::type *out, typename Op::type *total, bool tail)
{
	const unsigned nb = (unsigned)scan_parts(n_ub) - 1;
	const dim3 grid(nb ? nb : 1);
	hipLaunchKernelGGL((k_scan_part<Op, In>), grid, dim3(256), 0, st, in, part);
	hipLaunchKernelGGL((k_scan_top<Op, In>), dim3(1), dim3(256), 0, st, in, part, total);
	hipLaunchKernelGGL((k_scan_apply<Op, In>), grid, dim3(256), 0, st, in, (const typename Op::type*)part, out, tail ? 1 : 0);
}

} // namespace rb2
