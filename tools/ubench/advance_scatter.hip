// advance_scatter.hip -- what does the store side of k_advance cost?  n strings in tiles of 512, two per thread of a 256-thread block
// (x = h * 256 + thread), a random symbol in {1..4} per string plus 1 % of symbol 0 (a string that is done: not stored).  Per string:
// read 8 bytes (W) + 4 (L) + 1 (A), write 8 + 4 + 1 at the place a stable partition by symbol gives it: dst[a] + (strings with a in
// front of the tile: tpre) + (the same inside the tile, from ballots in LDS as group_setup / group_member have them), with
//   a  the direct scatter: every store instruction of a wave falls into four or five runs of ~16 lanes
//   b  through LDS: the tile's strings are laid down run by run, then thread j writes records j and j + 256 -- consecutive lanes on
//      consecutive addresses, a wave crosses a run boundary at most five times per tile instead of four times per instruction
// Same loads, same ballots and barriers in both; b has one more barrier and the LDS round trip.  hipEvent time per launch, median of 21.
// hipcc --offload-arch=gfx950 -O3 -o advance_scatter advance_scatter.hip && ./advance_scatter
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <vector>
#include <algorithm>
#define CHK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

constexpr int TILE = 512;
struct Tabs { uint32_t dst[6]; };

template <bool STAGE> __global__ __launch_bounds__(256) void k_scatter(const uint64_t *W, const uint32_t *L, const uint8_t *A, const uint32_t *tpre, Tabs tb,
		uint64_t *W2, uint32_t *L2, uint8_t *A2, uint32_t n)
{
	__shared__ uint64_t bal[8][6];
	__shared__ uint32_t cpre[9][6], s_tpre[6];
	__shared__ uint64_t s_w[STAGE ? TILE : 1]; __shared__ uint32_t s_l[STAGE ? TILE : 1]; __shared__ uint8_t s_a[STAGE ? TILE : 1];
	const uint32_t tile = blockIdx.x, base = tile * TILE;
	const int ln = threadIdx.x & 63, w = threadIdx.x >> 6;
	const uint32_t nval = min((uint32_t)TILE, n - base);
	uint64_t wv[2]; uint32_t lv[2]; int sym[2];
#pragma unroll
	for (int h = 0; h < 2; ++h) {
		const uint32_t x = h * 256 + threadIdx.x;
		wv[h] = 0; lv[h] = 0; sym[h] = 7;
		if (x < nval) { wv[h] = W[base + x]; lv[h] = L[base + x]; sym[h] = A[base + x] & 7; }
	}
	if (threadIdx.x < 6) s_tpre[threadIdx.x] = tb.dst[threadIdx.x] + tpre[tile * 6 + threadIdx.x];   // where the tile's strings with symbol a go
#pragma unroll
	for (int h = 0; h < 2; ++h) {
		uint64_t bm[6];
#pragma unroll
		for (int s = 0; s < 6; ++s) bm[s] = __ballot(sym[h] == s);
		if (ln == 0) {
#pragma unroll
			for (int s = 0; s < 6; ++s) bal[h * 4 + w][s] = bm[s];
		}
	}
	__syncthreads();
	if (threadIdx.x < 6) {
		const int s = threadIdx.x;
		uint32_t run = 0;
		for (int c = 0; c < 8; ++c) { cpre[c][s] = run; run += __popcll(bal[c][s]); }
		cpre[8][s] = run;
	}
	__syncthreads();
	uint32_t rs[7];                                             // where the run of symbol a starts among the tile's stored strings (symbol 0 is not stored)
	if (STAGE) {
		rs[0] = rs[1] = 0;
#pragma unroll
		for (int s = 1; s < 6; ++s) rs[s + 1] = rs[s] + cpre[8][s];
	}
#pragma unroll
	for (int h = 0; h < 2; ++h) {
		const int x = h * 256 + threadIdx.x, a = sym[h];
		if (a == 0 || a == 7) continue;
		const uint32_t pt = cpre[x >> 6][a] + __popcll(bal[x >> 6][a] & ((1ull << (x & 63)) - 1));   // strings with a in front of mine inside the tile
		const uint64_t wn = wv[h] + 1; const uint32_t l = lv[h] + pt;
		if (STAGE) {
			uint32_t r = 0;
#pragma unroll
			for (int s = 1; s < 6; ++s) r = a == s ? rs[s] : r;
			s_w[r + pt] = wn; s_l[r + pt] = l; s_a[r + pt] = (uint8_t)(wn & 7);
		} else {
			const uint32_t d = s_tpre[a] + pt;
			W2[d] = wn; L2[d] = l; A2[d] = (uint8_t)(wn & 7);
		}
	}
	if (STAGE) {
		__syncthreads();
#pragma unroll
		for (int h = 0; h < 2; ++h) {
			const uint32_t j = h * 256 + threadIdx.x;
			if (j >= rs[6]) continue;
			int a = 1; uint32_t r = rs[1];
#pragma unroll
			for (int s = 2; s < 6; ++s) if (j >= rs[s]) { a = s; r = rs[s]; }
			const uint32_t d = s_tpre[a] + (j - r);
			W2[d] = s_w[j]; L2[d] = s_l[j]; A2[d] = s_a[j];
		}
	}
}

static uint64_t splitmix(uint64_t k) { uint64_t z = (k + 1) * 0x9E3779B97F4A7C15ull; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }

int main()
{
	const uint32_t n = 34u * 1000 * 1000 + 77;                  // (a last tile that is not full)
	const uint32_t nt = (n + TILE - 1) / TILE;
	std::vector<uint8_t> hA(n); std::vector<uint32_t> htpre((size_t)nt * 6);
	uint64_t tot[6] = { 0, 0, 0, 0, 0, 0 };
	for (uint32_t i = 0; i < n; ++i) {
		if (i % TILE == 0) for (int s = 0; s < 6; ++s) htpre[(size_t)(i / TILE) * 6 + s] = (uint32_t)tot[s];
		const uint64_t z = splitmix(i);
		hA[i] = (z >> 32) % 100 == 0 ? 0 : 1 + (uint8_t)(z & 3);
		++tot[hA[i]];
	}
	Tabs tb; uint32_t run = 0;
	for (int s = 0; s < 6; ++s) { tb.dst[s] = run; if (s) run += (uint32_t)tot[s]; }
	const uint32_t nout = run;
	uint64_t *W, *W2; uint32_t *L, *L2, *tpre; uint8_t *A, *A2;
	CHK(hipMalloc(&W, (size_t)n * 8)); CHK(hipMalloc(&W2, (size_t)n * 8)); CHK(hipMalloc(&L, (size_t)n * 4)); CHK(hipMalloc(&L2, (size_t)n * 4));
	CHK(hipMalloc(&A, n)); CHK(hipMalloc(&A2, n)); CHK(hipMalloc(&tpre, (size_t)nt * 24));
	CHK(hipMemcpy(A, hA.data(), n, hipMemcpyHostToDevice)); CHK(hipMemcpy(tpre, htpre.data(), (size_t)nt * 24, hipMemcpyHostToDevice));
	CHK(hipMemset(W, 3, (size_t)n * 8)); CHK(hipMemset(L, 1, (size_t)n * 4));
	hipEvent_t e0, e1; CHK(hipEventCreate(&e0)); CHK(hipEventCreate(&e1));
	auto run1 = [&](int mode) {
		if (mode == 0) hipLaunchKernelGGL(k_scatter<false>, dim3(nt), dim3(256), 0, 0, W, L, A, tpre, tb, W2, L2, A2, n);
		else hipLaunchKernelGGL(k_scatter<true>, dim3(nt), dim3(256), 0, 0, W, L, A, tpre, tb, W2, L2, A2, n);
	};
	// the two variants write the same thing
	std::vector<uint32_t> r0(nout), r1(nout); std::vector<uint8_t> a0(nout), a1(nout);
	CHK(hipMemset(L2, 0xff, (size_t)n * 4)); CHK(hipMemset(A2, 0xff, n)); run1(0);
	CHK(hipMemcpy(r0.data(), L2, (size_t)nout * 4, hipMemcpyDeviceToHost)); CHK(hipMemcpy(a0.data(), A2, nout, hipMemcpyDeviceToHost));
	CHK(hipMemset(L2, 0xff, (size_t)n * 4)); CHK(hipMemset(A2, 0xff, n)); run1(1);
	CHK(hipMemcpy(r1.data(), L2, (size_t)nout * 4, hipMemcpyDeviceToHost)); CHK(hipMemcpy(a1.data(), A2, nout, hipMemcpyDeviceToHost));
	printf("%u strings, %u stored; a and b %s\n", n, nout, r0 == r1 && a0 == a1 ? "agree" : "DIFFER");
	const char *name[2] = { "a  direct scatter", "b  staged in LDS, whole runs" };
	const int NREP = 21;
	for (int rep = 0; rep < 3; ++rep) for (int mode = 0; mode < 2; ++mode) {
		run1(mode);
		std::vector<float> t(NREP);
		for (int i = 0; i < NREP; ++i) {
			CHK(hipEventRecord(e0)); run1(mode); CHK(hipEventRecord(e1)); CHK(hipEventSynchronize(e1));
			CHK(hipEventElapsedTime(&t[i], e0, e1));
		}
		std::sort(t.begin(), t.end());
		const double bytes = 13.0 * n + 13.0 * nout;
		printf("%-32s median %.4f ms (min %.4f, max %.4f) = %.2f TB/s\n", name[mode], t[NREP / 2], t[0], t[NREP - 1], bytes / t[NREP / 2] / 1e9);
	}
	return 0;
}
