// sym_pair.hip -- does a 256-thread block that takes TWO 512-string tiles per barrier stream faster than one that takes one?  The accesses of the
// fused k_sym<false, uint32_t> (rb2_kernels.h): per string read 1 byte (A) + 4 bytes (L) + the predecessor's L (same lines), write 1 byte (A) + 4
// bytes (INS_E) + 1 byte (INS_A); seven ballots per 64 strings into an LDS table, ONE barrier, a per-tile summary written by six threads, then the
// stores -- 11 bytes of traffic per string as in elem_stream.hip.  n = 34 M strings (a dense round of the bench job).
//   1  one tile per block   (the kernel up to round 7)
//   2  two tiles per block: all loads of both tiles issued before anything is looked at, one barrier per 1024 strings
// hipcc --offload-arch=gfx950 -O3 -o sym_pair sym_pair.hip && ./sym_pair
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#define CHK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

template <int NT> __global__ __launch_bounds__(256) void k(const uint8_t *A, const uint32_t *L, uint8_t *A2, uint32_t *E, uint8_t *IA, uint32_t *REC, uint64_t n)
{
	__shared__ uint64_t s_bal[NT][8][6], s_head[NT][8];
	__shared__ __align__(16) uint32_t s_ok[NT][4];
	const int ln = threadIdx.x & 63, w = threadIdx.x >> 6;
	const uint64_t ntile = (n + 511) / 512, tile0 = (uint64_t)blockIdx.x * NT;
	if (tile0 >= ntile) return;
	uint32_t a[NT][2], l[NT][2], lp[NT][2], nval[NT];
#pragma unroll
	for (int q = 0; q < NT; ++q) {
		const uint64_t base = (tile0 + q) * 512;
		nval[q] = base < n ? (uint32_t)(n - base < 512 ? n - base : 512) : 0u;
#pragma unroll
		for (int h = 0; h < 2; ++h) {
			const uint32_t x = h * 256 + threadIdx.x;
			a[q][h] = 7; l[q][h] = 0; lp[q][h] = 0;
			if (x < nval[q]) { a[q][h] = A[base + x]; l[q][h] = L[base + x]; lp[q][h] = base + x ? L[base + x - 1] : 0u; }
		}
	}
#pragma unroll
	for (int q = 0; q < NT; ++q) {
		const uint64_t base = (tile0 + q) * 512;
		bool single = true;
#pragma unroll
		for (int h = 0; h < 2; ++h) {
			const uint32_t x = h * 256 + threadIdx.x;
			const int sym = (int)(a[q][h] & 7);
			const bool head = x < nval[q] && (base + x == 0 || l[q][h] != lp[q][h]);
			if (x < nval[q]) { A2[base + x] = (uint8_t)(sym | (head ? 0x80 : 0)); single = single && head; }
			uint64_t bm[6];
#pragma unroll
			for (int s = 0; s < 6; ++s) bm[s] = __builtin_amdgcn_ballot_w64(sym == s);
			const uint64_t hm = __builtin_amdgcn_ballot_w64(head);
			if (ln == 0) {
#pragma unroll
				for (int s = 0; s < 6; ++s) s_bal[q][h * 4 + w][s] = bm[s];
				s_head[q][h * 4 + w] = hm;
			}
		}
		const uint64_t sm = __builtin_amdgcn_ballot_w64(single);
		if (ln == 0) s_ok[q][w] = sm == ~0ull ? 1u : 0u;
	}
	__syncthreads();
#pragma unroll
	for (int q = 0; q < NT; ++q) {
		const uint64_t base = (tile0 + q) * 512;
		const uint4 okv = *(const uint4*)s_ok[q];
		if ((okv.x & okv.y & okv.z & okv.w) != 0) {
#pragma unroll
			for (int h = 0; h < 2; ++h) {
				const uint32_t x = h * 256 + threadIdx.x;
				if (x < nval[q]) { E[base + x] = l[q][h] - x; IA[base + x] = (uint8_t)(a[q][h] & 7); }
			}
		}
	}
	if (threadIdx.x < 6 * NT) {
		const int q = threadIdx.x / 6, s = threadIdx.x % 6;
		if (tile0 + q < ntile) {
			uint32_t run = 0;
#pragma unroll
			for (int c = 0; c < 8; ++c) run += __popcll(s_bal[q][c][s]);
			REC[(uint64_t)s * ntile + tile0 + q] = run + (uint32_t)__popcll(s_head[q][7]);
		}
	}
}

int main()
{
	const uint64_t n = 34ull * 1000 * 1000, ntile = (n + 511) / 512;
	uint8_t *A, *A2, *IA; uint32_t *L, *E, *REC;
	CHK(hipMalloc(&A, n)); CHK(hipMalloc(&A2, n)); CHK(hipMalloc(&IA, n)); CHK(hipMalloc(&L, n * 4)); CHK(hipMalloc(&E, n * 4)); CHK(hipMalloc(&REC, ntile * 6 * 4));
	CHK(hipMemset(A, 1, n));
	{	// L strictly increasing: every string is a group of its own, as from round ~14 of a batch on
		uint32_t *hl = (uint32_t*)malloc(n * 4);
		for (uint64_t i = 0; i < n; ++i) hl[i] = (uint32_t)(3 * i + 1);
		CHK(hipMemcpy(L, hl, n * 4, hipMemcpyHostToDevice)); free(hl);
	}
	hipEvent_t e0, e1; CHK(hipEventCreate(&e0)); CHK(hipEventCreate(&e1));
	const char *name[2] = { "one 512-string tile per 256-thread block, one barrier per 512", "two tiles per 256-thread block, one barrier per 1024" };
	for (int rep = 0; rep < 3; ++rep) for (int mode = 0; mode < 2; ++mode) {
		auto run = [&] {
			if (mode == 0) hipLaunchKernelGGL(k<1>, dim3((unsigned)ntile), dim3(256), 0, 0, A, L, A2, E, IA, REC, n);
			else hipLaunchKernelGGL(k<2>, dim3((unsigned)((ntile + 1) / 2)), dim3(256), 0, 0, A, L, A2, E, IA, REC, n);
		};
		run();
		CHK(hipEventRecord(e0));
		for (int i = 0; i < 20; ++i) run();
		CHK(hipEventRecord(e1)); CHK(hipEventSynchronize(e1));
		float ms; CHK(hipEventElapsedTime(&ms, e0, e1)); ms /= 20;
		printf("%-64s %.4f ms for %.1f M strings x 11 bytes = %.2f TB/s\n", name[mode], ms, n / 1e6, 11.0 * n / ms / 1e9);
	}
	return 0;
}
