// A serial .fmd encoder made ONLY of the functions of csrc/rb2_fmd_plan.h (width, code bits, header type and words, payload bits, the fit
// rule as a bisection over the prefix sum of the widths, the frame rule) against the host writer (csrc/host/fmd.c: rb2_fmd_push /
// rb2_fmd_finish / rb2_fmd_write), whole images byte for byte.  Run by tests/test_fmd_plan.py; "big" as argv[1] adds the stream that
// crosses a chunk of 2^23 words.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <vector>
#include "rb2_fmd_plan.h"
extern "C" {
#include "rb2_fmd.h"
}

struct Run { uint64_t l; uint32_t c; };
struct Events {            // what the model met in one stream; summed over the streams that were COMPARED with the writer (EV) and over the others (EVU)
	uint64_t word_end = 0;     // a code ended on the last bit of a word before the last one
	uint64_t bit_before = 0;   // ... on the bit before the block's last
	uint64_t exact = 0;        // ... on the block's last bit (from u == C - 64)
	uint64_t refused_exact = 0;   // a code that would have ended on the last bit from inside the last word and moved on
	uint64_t w64_at_c64 = 0, w64_at_0 = 0;   // a 64-bit code at u == C - 64 / at a block's first bit
	uint64_t trans[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};   // header type followed by header type
	uint64_t t16383 = 0, t16384 = 0, t30m = 0, t30 = 0;         // a block's total at the edges of the types
	uint64_t short_blocks = 0;  // last blocks of a chunk
	uint64_t undefined = 0;     // a 64-bit code right behind a code that ended on a word boundary: the writer shifts by 64 there (as rld0.c:145 does)
};
static Events EV, EVU;
static void add(Events &a, const Events &b)
{
	a.word_end += b.word_end; a.bit_before += b.bit_before; a.exact += b.exact; a.refused_exact += b.refused_exact;
	a.w64_at_c64 += b.w64_at_c64; a.w64_at_0 += b.w64_at_0;
	for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) a.trans[i][j] += b.trans[i][j];
	a.t16383 += b.t16383; a.t16384 += b.t16384; a.t30m += b.t30m; a.t30 += b.t30;
	a.short_blocks += b.short_blocks; a.undefined += b.undefined;
}

static void put64(std::vector<uint8_t> &v, uint64_t x) { for (int i = 0; i < 8; ++i) v.push_back((uint8_t)(x >> (8 * i))); }

// the image of a stream of maximal runs (neighbours differ)
template <typename WT> static std::vector<uint8_t> model(const std::vector<Run> &R, Events &EV)
{
	const uint64_t n = R.size();
	std::vector<WT> W(n + 1);
	W[0] = 0;
	for (uint64_t j = 0; j < n; ++j) W[j + 1] = (WT)(W[j] + fmds_width(R[j].l));
	std::vector<uint64_t> words;
	std::vector<uint64_t> hS;                                  // per header k >= 1: nothing but what the frame rule needs
	std::vector<uint64_t> hcum;                                // 6 cumulative counts per header
	uint64_t prev[7] = {0, 0, 0, 0, 0, 0, 0}, cum[7] = {0, 0, 0, 0, 0, 0, 0};
	uint64_t i = 0, blk = 0;
	uint32_t type = 0, ptype = 0;
	for (;;) {
		uint64_t b[FMDS_BW];
		for (uint32_t k = 0; k < FMDS_BW; ++k) b[k] = k < 7 ? fmds_hdr_word(type, prev, k) : 0;
		for (uint32_t k = fmds_hdr_words(type); k < 7; ++k) b[k] = 0;
		if (blk) {
			for (int a = 0; a < 7; ++a) cum[a] += prev[a];
			hS.push_back(cum[0]);
			for (int a = 1; a < 7; ++a) hcum.push_back(cum[a]);
			++EV.trans[ptype][type];
			if (prev[0] == 16383) ++EV.t16383;
			if (prev[0] == 16384) ++EV.t16384;
			if (prev[0] == (1ull << 30) - 1) ++EV.t30m;
			if (prev[0] == 1ull << 30) ++EV.t30;
		}
		const uint32_t hw = fmds_hdr_words(type);
		if (i == n && blk) {                                   // the closing header (an empty stream: block 0 is all zero, the closing header is block 1)
			for (uint32_t k = 0; k < hw; ++k) words.push_back(b[k]);
			break;
		}
		const bool last = fmds_chunk_last(blk);
		if (last) ++EV.short_blocks;
		const uint32_t C = fmds_payload_bits(type, last);
		bool complete;
		uint64_t e = fmds_block_end(W.data(), i, n, C, &complete);
		if (!complete) e = n;
		uint64_t cnt[7] = {0, 0, 0, 0, 0, 0, 0};
		for (uint64_t j = i; j < e; ++j) {
			const uint32_t u = (uint32_t)(W[j] - W[i]), w = fmds_width(R[j].l);
			const FmdsPlace p = fmds_place(u, fmds_code(R[j].l, R[j].c), w);
			b[hw + p.wi] |= p.hi;
			if (p.spill) b[hw + p.wi + 1] |= p.lo;
			cnt[0] += R[j].l; cnt[1 + R[j].c] += R[j].l;
			if ((u + w) % 64 == 0 && u + w < C) ++EV.word_end;
			if (u + w == C - 1) ++EV.bit_before;
			if (u + w == C) ++EV.exact;
			if (w == 64 && u + 64 == C && u > 0) ++EV.w64_at_c64;
			if (w == 64 && u == 0) ++EV.w64_at_0;
			if (w == 64 && u > 0 && u % 64 == 0) ++EV.undefined;
		}
		if (complete && e < n && (uint32_t)(W[e] - W[i]) + fmds_width(R[e].l) == C) ++EV.refused_exact;
		for (uint32_t k = 0; k < FMDS_BW; ++k) words.push_back(b[k]);
		memcpy(prev, cnt, sizeof(cnt));
		ptype = type; type = fmds_type(cnt[0]);
		i = e; ++blk;
	}
	const uint64_t n_bytes = words.size() * 8, total = cum[0];
	const int ibits = fmds_ibits(total, n_bytes);
	const uint64_t n_frames = fmds_n_frames(total, ibits);
	std::vector<uint64_t> fr(n_frames * 7, 0);
	for (uint64_t k = 0; k < hS.size(); ++k) {                 // the last header of a frame wins
		const uint64_t f = fmds_frame_of(hS[k], ibits);
		if (f >= n_frames) continue;
		fr[f * 7] = (k + 1) * FMDS_BW;
		for (int a = 0; a < 6; ++a) fr[f * 7 + 1 + a] = hcum[k * 6 + a];
	}
	for (uint64_t f = 1; f < n_frames; ++f) if (fr[f * 7] == 0) memcpy(&fr[f * 7], &fr[(f - 1) * 7], 56);
	std::vector<uint8_t> img;
	img.reserve((size_t)fmds_image_size(n_bytes, n_frames));
	img.push_back('R'); img.push_back('L'); img.push_back('D'); img.push_back(3);
	const uint32_t ab = 6u << 16 | 3u;
	for (int k = 0; k < 4; ++k) img.push_back((uint8_t)(ab >> (8 * k)));
	put64(img, 0); put64(img, n_bytes); put64(img, n_frames);
	for (int a = 1; a < 7; ++a) put64(img, cum[a]);
	for (uint64_t w : words) put64(img, w);
	for (uint64_t w : fr) put64(img, w);
	if (img.size() != fmds_image_size(n_bytes, n_frames)) { printf("FAIL image size\n"); exit(1); }
	return img;
}

static std::vector<uint8_t> oracle(const std::vector<Run> &R)
{
	rb2_fmd_t *f = rb2_fmd_init();
	for (const Run &r : R) rb2_fmd_push(f, (int64_t)r.l, (int)r.c);
	rb2_fmd_finish(f);
	char *buf = nullptr; size_t len = 0;
	FILE *fp = open_memstream(&buf, &len);
	if (rb2_fmd_write(f, fp) != 0) { printf("FAIL oracle write\n"); exit(1); }
	fclose(fp);
	std::vector<uint8_t> img(buf, buf + len);
	free(buf);
	rb2_fmd_destroy(f);
	return img;
}

static uint64_t n_streams[8], n_undefined;
template <typename WT = uint64_t> static void check(int kind, const std::vector<Run> &R)
{
	for (size_t j = 1; j < R.size(); ++j) if (R[j].c == R[j - 1].c || R[j].l == 0) { printf("FAIL bad test stream\n"); exit(1); }
	Events E;
	const std::vector<uint8_t> a = model<WT>(R, E), b = oracle(R);
	if (E.undefined) { add(EVU, E); ++n_undefined; return; }     // no statement of the format to compare with: counted, not compared, and its events count for nothing
	add(EV, E);
	if (a != b) {
		size_t d = 0;
		while (d < a.size() && d < b.size() && a[d] == b[d]) ++d;
		printf("FAIL kind %d, %zu runs: images of %zu and %zu bytes differ at byte %zu\n", kind, R.size(), a.size(), b.size(), d); for (size_t j = 0; j < R.size() && j < 200; ++j) printf(" %llu:%u", (unsigned long long)R[j].l, R[j].c); printf("\n");
		exit(1);
	}
	++n_streams[kind];
}

static uint64_t rng_s = 0x9E3779B97F4A7C15ull;
static uint64_t rng() { rng_s ^= rng_s << 13; rng_s ^= rng_s >> 7; rng_s ^= rng_s << 17; return rng_s; }
static void ones(std::vector<Run> &R, int n) { for (int k = 0; k < n; ++k) R.push_back({1, R.empty() ? 1u : (R.back().c == 1 ? 2u : 1u)}); }
static void one(std::vector<Run> &R, uint64_t l) { R.push_back({l, R.empty() ? 3u : (R.back().c == 3 ? 4u : 3u)}); }

int main(int argc, char **argv)
{
	const bool big = argc > 1 && strcmp(argv[1], "big") == 0;
	std::vector<uint64_t> probes;
	for (uint64_t l = 1; l <= 70; ++l) probes.push_back(l);
	for (int k = 7; k <= 50; ++k) { probes.push_back((1ull << k) - 1); probes.push_back(1ull << k); probes.push_back((1ull << k) + 1); }
	// kind 0: every probe length alone, and the empty stream
	check(0, {});
	for (uint64_t l : probes) for (uint32_t c = 0; c < 6; c += 5) check(0, {{l, c}});
	// kind 1: all-ones runs of alternating symbols
	for (int n : {2, 94, 95, 96, 97, 191, 1000, 5000}) { std::vector<Run> R; ones(R, n); check(1, R); }
	// kind 2: a ones in front of every probe length, ones behind it: every alignment of every width at every edge of a block
	for (int a = 0; a <= 96; ++a)
		for (uint64_t l : probes) { std::vector<Run> R; ones(R, a); one(R, l); ones(R, 12); check(2, R); }
	// kind 3: 64-bit codes one after the other and between shorter ones (a 64-bit code at a block's first bit, at u == C - 64)
	for (int a = 0; a <= 96; ++a)
		for (int rep = 1; rep <= 7; ++rep) { std::vector<Run> R; ones(R, a); for (int k = 0; k < rep; ++k) one(R, (1ull << 50) + (uint64_t)k); ones(R, 3); one(R, 1ull << 50); check(3, R); }
	// kind 4: totals at the edges of the header types.  A block behind one of >= 2^30 symbols has one payload word: it holds a run of T symbols
	// alone when a run of 2^30 follows it (its code does not fit behind T's), so the next header holds exactly T
	for (uint64_t T : {16383ull, 16384ull, (1ull << 30) - 1, 1ull << 30, 5ull, 20000ull})
		for (int a = 0; a < 3; ++a) {
			std::vector<Run> R;
			ones(R, a * 40);
			for (int k = 0; k < 6; ++k) { one(R, 1ull << 30); R.push_back({T, 5}); }
			ones(R, 200); one(R, 20000); ones(R, 3); one(R, 20000); one(R, 16384); ones(R, 100);
			check(4, R);
		}
	{	// ... and a long mixture, so that every type follows every other
		const uint64_t L[8] = {1, 5, 16383, 16384, 20000, (1ull << 30) - 1, 1ull << 30, (1ull << 30) + 5};
		std::vector<Run> R;
		for (int k = 0; k < 20000; ++k) { const uint32_t c = R.empty() ? 0u : (R.back().c + 1 + (uint32_t)(rng() % 5)) % 6; R.push_back({L[rng() % 8], c}); }
		check(4, R);
	}
	// kind 5: random runs, lengths drawn log-uniformly
	{
		std::vector<Run> R;
		for (int k = 0; k < 100000; ++k) {
			const int e = (int)(rng() % 45);
			const uint64_t l = (1ull << e) | (rng() & ((1ull << e) - 1));
			const uint32_t c = R.empty() ? 0u : (R.back().c + 1 + (uint32_t)(rng() % 5)) % 6;
			R.push_back({l, c});
		}
		check(5, R);
	}
	// kind 6: alternating single symbols across the end of a chunk of 2^23 words (95 runs per block)
	if (big) { std::vector<Run> R; R.reserve(100700000); ones(R, 100700000); check<uint32_t>(6, R); }
	bool all = true;
	for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) all = all && EV.trans[a][b] > 0;
	const bool edges = EV.t16383 && EV.t16384 && EV.t30m && EV.t30;
	// from compared streams only.  A 64-bit code at u == C - 64 > 0 always stands behind a word boundary (C is a multiple of 64), where the writer
	// shifts by 64: no compared stream can hold one, the model-only count says how many the model encoded; at C == 64 (u == 0) it is compared (w64_at_0, exact)
	const bool ev = EV.word_end && EV.bit_before && EV.exact && EV.refused_exact && EV.w64_at_0 && EV.w64_at_c64 == 0;
	if (!all || !edges || !ev || (big && EV.short_blocks != 1)) {
		printf("FAIL coverage: transitions %d, edges %d (%llu %llu %llu %llu), events %llu %llu %llu %llu %llu %llu, short blocks %llu\n", (int)all, (int)edges,
			(unsigned long long)EV.t16383, (unsigned long long)EV.t16384, (unsigned long long)EV.t30m, (unsigned long long)EV.t30,
			(unsigned long long)EV.word_end, (unsigned long long)EV.bit_before, (unsigned long long)EV.exact, (unsigned long long)EV.refused_exact,
			(unsigned long long)EV.w64_at_c64, (unsigned long long)EV.w64_at_0, (unsigned long long)EV.short_blocks);
		return 1;
	}
	printf("FMD PLAN OK: alone %llu ones %llu aligned %llu wide %llu types %llu random %llu chunk %llu transitions 9 edges 4 events 5 undefined %llu model_only_w64_at_c64 %llu\n",
		(unsigned long long)n_streams[0], (unsigned long long)n_streams[1], (unsigned long long)n_streams[2], (unsigned long long)n_streams[3],
		(unsigned long long)n_streams[4], (unsigned long long)n_streams[5], (unsigned long long)n_streams[6], (unsigned long long)n_undefined, (unsigned long long)EVU.w64_at_c64);
	return 0;
}
