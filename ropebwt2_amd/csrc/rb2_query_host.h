// Host side of the FM-index queries (kernels: rb2_query.h; the launch arithmetic: rb2_query_plan.h, rb2_kmer_plan.h).  Included from rb2_engine.hip, whose
// handle, buffers and checks it uses.  Four helpers carry every query: qlaunch (one launch of a kernel in the layout of the index),
// stage_inputs (a chunk's inputs to the device), staged_records (the chunked loop of the host variants that return records) and
// dev_chunks (the chunked loop of the device-pointer variants).  Beside them: env_i64 reads the caps the environment may set, stacked_search
// and stacked_search_dev are the whole host side of the searches that keep a path stack per query length (rb2_hip_approx, rb2_hip_approx_ed),
// and BatchSource streams the strings of one index into another (rb2_hip_merge, rb2_hip_correct_into).
#pragma once
#include "rb2_query_plan.h"
#include "rb2_edit_plan.h"
#include "rb2_kmer_plan.h"
#include "rb2_graph_plan.h"

/* a number the environment may set, read on every call: its value when it is positive, dflt when it is unset, no number or not positive */
static int64_t env_i64(const char *name, int64_t dflt)
{
	const char *e = getenv(name);
	const int64_t v = e ? atoll(e) : 0;
	return v > 0 ? v : dflt;
}

/* queries per launch: 16 threads each, so 2^24 stay far below the 2^32 threads of one launch; RB2_QUERY_CHUNK lowers it (tests of the chunking) */
static int64_t query_chunk()
{
	const int64_t CH = 1 << 24;
	const char *e = getenv("RB2_QUERY_CHUNK");
	const int64_t v = e ? atoll(e) : 0;
	return v > 0 ? std::min(v, CH) : CH;
}

/* what every query does first: wait for a lazy insert, refuse a shard, build the piece table of the index as it is now */
static void query_begin(rb2_hip_t *h, const char *who)
{
	finish_pending(h);
	HIPCHK(hipSetDevice(h->dev));
	if (h->nranks > 1) rb2_fatal("[rb2_hip] %s: this handle holds only its own sub-ropes of a sharded index; queries need the whole index on one engine\n", who);
	require_plain(h, who);
	h->qtab.ensure(1);
	hipLaunchKernelGGL(k_qtab, dim3(1), dim3(64), 0, h->st, (const Ctl*)h->ctl, h->side, h->pool[h->pside].view(), h->qtab.p);
	HIPCHK(hipGetLastError());
}

/* one launch of a query kernel, one DPP row (16 lanes) for each of rows: the instantiation for the layout of the index, on the handle's
 * stream, the piece table and the pool in front of the kernel's own arguments a */
template <typename... P, typename... A>
static void qlaunch(rb2_hip_t *h, void (*sparse)(const QTab*, PoolView, P...), void (*dense)(const QTab*, PoolView, P...), uint64_t rows, A... a)
{
	const auto k = h->sparse ? sparse : dense;
	hipLaunchKernelGGL(k, dim3((unsigned)cdiv(rows, QPB)), dim3(256), 0, h->st, (const QTab*)h->qtab.p, h->pool[h->pside].view(), static_cast<P>(a)...);
	HIPCHK(hipGetLastError());
}

/* the _dev variants that take packed strings: launch(i0, nc) for the items [i0, i0 + nc) of every chunk, nothing staged and no synchronise */
template <typename F>
static void dev_chunks(int64_t n, F launch)
{
	const int64_t CH = query_chunk();
	for (int64_t i0 = 0; i0 < n; i0 += CH) launch(i0, std::min(CH, n - i0));
}

/* the inputs of a host variant, in host memory: n packed strings (w == 0: bytes, and v = their n + 1 offsets) or n tuples of w int64 (v;
 * NULL: the items are their own numbers and nothing is copied) */
struct QInput { const uint8_t *bytes; const int64_t *v; int w; };
/* a chunk of them on the device: v as it was cut from the host's (offsets still count from the first byte of the whole input, base of them
 * in front of bytes; tuples: base = the number of the chunk's first item, v = NULL when the host gave none), and tail, room behind v for
 * what the kernel writes per item beside its records */
struct QStaged { const uint8_t *bytes; const int64_t *v; int64_t base; int64_t *tail; };

static void check_offsets(const char *who, const char *what, int64_t n, const int64_t *off)
{
	for (int64_t i = 0; i < n; ++i)
		if (off[i + 1] < off[i] || off[0] < 0) { rb2_fatal("[rb2_hip] %s: %s offsets must be non-negative and non-decreasing (off[%lld])\n", who, what, (long long)i); }
}

/* the items [i0, i0 + nc) of in into qin (and qbytes), with tail more int64 behind them; asynchronous on the handle's stream */
static QStaged stage_inputs(rb2_hip_t *h, const QInput &in, int64_t i0, int64_t nc, int64_t tail)
{
	const int64_t nw = in.w ? nc * in.w : nc + 1, first = in.w ? i0 * in.w : i0;
	int64_t base = in.w ? i0 : 0;
	h->qin.ensure((size_t)(nw + tail));
	if (in.v) HIPCHK(hipMemcpyAsync(h->qin.p, in.v + first, (size_t)nw * 8, hipMemcpyHostToDevice, h->st));
	if (!in.w) {
		base = in.v[i0];
		const int64_t nb = in.v[i0 + nc] - base;
		h->qbytes.ensure((size_t)std::max<int64_t>(nb, 1));
		if (nb) HIPCHK(hipMemcpyAsync(h->qbytes.p, in.bytes + base, (size_t)nb, hipMemcpyHostToDevice, h->st));
	}
	return {h->qbytes.p, in.v ? h->qin.p : nullptr, base, h->qin.p + nw};
}

/* the host variants with one fixed result of words int64 per item: launch(nc, staged inputs, results) per chunk, one synchronise each */
template <typename F>
static void staged_results(rb2_hip_t *h, int64_t n, const QInput &in, int words, int64_t *out, F launch)
{
	const int64_t CH = query_chunk();
	for (int64_t i0 = 0; i0 < n; i0 += CH) {
		const int64_t nc = std::min(CH, n - i0);
		const QStaged s = stage_inputs(h, in, i0, nc, 0);
		h->qout.ensure((size_t)nc * words);
		launch(nc, s, h->qout.p);
		HIPCHK(hipMemcpyAsync(out + i0 * words, h->qout.p, (size_t)nc * words * 8, hipMemcpyDeviceToHost, h->st));
		HIPCHK(hipStreamSynchronize(h->st));
	}
}

/* the host variants with up to cap (>= 1) records of words int64 per item and a count: launch(nc, staged inputs, records, counts) per chunk of
 * at most QUERY_STAGE_BYTES of records (one item when a single one has more), one synchronise each.  The records no item writes come
 * back as zeros; returns the records stored, min(stored_of(cnt), cap) over the items (stored_of: max(cnt, 0) unless the family says otherwise) */
template <typename F, typename S>
static int64_t staged_records(rb2_hip_t *h, int64_t n, const QInput &in, int words, int64_t cap, int64_t *rec, int64_t *cnt, F launch, S stored_of)
{
	const int64_t CH = record_chunk(query_chunk(), 8 * words * cap);
	int64_t stored = 0;
	for (int64_t i0 = 0; i0 < n; i0 += CH) {
		const int64_t nc = std::min(CH, n - i0);
		const size_t bytes = (size_t)(nc * cap) * words * 8;
		const QStaged s = stage_inputs(h, in, i0, nc, nc);
		h->qout.ensure(bytes / 8);
		HIPCHK(hipMemsetAsync(h->qout.p, 0, bytes, h->st));
		launch(nc, s, h->qout.p, s.tail);
		HIPCHK(hipMemcpyAsync(cnt + i0, s.tail, (size_t)nc * 8, hipMemcpyDeviceToHost, h->st));
		HIPCHK(hipMemcpyAsync(rec + i0 * cap * words, h->qout.p, bytes, hipMemcpyDeviceToHost, h->st));
		HIPCHK(hipStreamSynchronize(h->st));
		for (int64_t i = i0; i < i0 + nc; ++i) stored += std::min(stored_of(cnt[i]), cap);
	}
	return stored;
}

template <typename F>
static int64_t staged_records(rb2_hip_t *h, int64_t n, const QInput &in, int words, int64_t cap, int64_t *rec, int64_t *cnt, F launch)
{
	return staged_records(h, n, in, words, cap, rec, cnt, launch, [](int64_t c) { return std::max<int64_t>(c, 0); });
}

/* ---- backward search, extend, extract: one DPP row of 16 lanes per query ---- */

static void launch_bsearch(rb2_hip_t *h, int64_t n, const uint8_t *pat, const int64_t *off, int64_t base, int64_t *out)
{
	qlaunch(h, k_bsearch<true>, k_bsearch<false>, (uint64_t)n, pat, off, base, n, out);
}

void rb2_hip_backward_search(rb2_hip_t *h, int64_t n, const uint8_t *pat, const int64_t *off, int64_t *out)
{
	query_begin(h, "backward_search");
	if (n <= 0) return;
	check_offsets("backward_search", "pattern", n, off);
	staged_results(h, n, {pat, off, 0}, 3, out, [&](int64_t nc, const QStaged &s, int64_t *d_out) { launch_bsearch(h, nc, s.bytes, s.v, s.base, d_out); });
}

void rb2_hip_backward_search_dev(rb2_hip_t *h, int64_t n, const uint8_t *pat, const int64_t *off, int64_t *out)
{
	query_begin(h, "backward_search_dev");
	dev_chunks(n, [&](int64_t i0, int64_t nc) { launch_bsearch(h, nc, pat, off + i0, 0, out + 3 * i0); });
}

void rb2_hip_extend(rb2_hip_t *h, int64_t n, const int64_t *ik, int is_back, int64_t *ok)
{
	query_begin(h, "extend");
	if (n <= 0) return;
	is_back = is_back ? 1 : 0;
	staged_results(h, n, {nullptr, ik, 3}, 18, ok, [&](int64_t nc, const QStaged &s, int64_t *d_ok) {
		qlaunch(h, k_extend<true>, k_extend<false>, (uint64_t)nc, s.v, is_back, nc, d_ok); });
}

int64_t rb2_hip_extract(rb2_hip_t *h, int64_t n, const int64_t *rows, int64_t max_len, uint8_t *out, int64_t *len)
{
	query_begin(h, "extract");
	if (n <= 0) return 0;
	if (max_len < 0) max_len = 0;
	int64_t CH = query_chunk();
	if (max_len > 0) CH = record_chunk(CH, max_len);
	h->qbytes.ensure((size_t)std::max<int64_t>(std::min(CH, n) * max_len, 1));
	int64_t fit = 0;
	for (int64_t i0 = 0; i0 < n; i0 += CH) {
		const int64_t nc = std::min(CH, n - i0);
		const QStaged s = stage_inputs(h, {nullptr, rows, 1}, i0, nc, nc);
		qlaunch(h, k_extract<true>, k_extract<false>, (uint64_t)nc, s.v, nc, max_len, h->qbytes.p, s.tail);
		HIPCHK(hipMemcpyAsync(len + i0, s.tail, (size_t)nc * 8, hipMemcpyDeviceToHost, h->st));
		if (nc * max_len) HIPCHK(hipMemcpyAsync(out + i0 * max_len, h->qbytes.p, (size_t)(nc * max_len), hipMemcpyDeviceToHost, h->st));
		HIPCHK(hipStreamSynchronize(h->st));
		for (int64_t i = i0; i < i0 + nc; ++i)                  // the walk spells a string from its last symbol: text order is the reverse
			if (len[i] >= 0) { std::reverse(out + i * max_len, out + i * max_len + len[i]); ++fit; }
	}
	return fit;
}

/* ---- super-maximal exact matches (k_smem) ---- */

static void launch_smem(rb2_hip_t *h, int64_t n, const uint8_t *qry, const int64_t *off, int64_t base, int64_t min_len, int64_t min_occ, int64_t max_mems,
                        int64_t *mem, int64_t *cnt)
{
	qlaunch(h, k_smem<true>, k_smem<false>, (uint64_t)n, qry, off, base, n, min_len, min_occ, max_mems, mem, cnt);
}

static void smem_check(const char *who, int64_t min_len, int64_t min_occ, int64_t max_mems)
{
	if (min_len < 1 || min_occ < 1 || max_mems < 1)
		rb2_fatal("[rb2_hip] %s: min_len, min_occ and max_mems must be at least 1 (got %lld, %lld, %lld)\n", who, (long long)min_len, (long long)min_occ, (long long)max_mems);
}

int64_t rb2_hip_smem(rb2_hip_t *h, int64_t n, const uint8_t *qry, const int64_t *off, int64_t min_len, int64_t min_occ, int64_t max_mems, int64_t *mem, int64_t *cnt)
{
	query_begin(h, "smem");
	if (n <= 0) return 0;
	smem_check("smem", min_len, min_occ, max_mems);
	check_offsets("smem", "query", n, off);
	return staged_records(h, n, {qry, off, 0}, 5, max_mems, mem, cnt, [&](int64_t nc, const QStaged &s, int64_t *d_mem, int64_t *d_cnt) {
		launch_smem(h, nc, s.bytes, s.v, s.base, min_len, min_occ, max_mems, d_mem, d_cnt); });
}

void rb2_hip_smem_dev(rb2_hip_t *h, int64_t n, const uint8_t *qry, const int64_t *off, int64_t min_len, int64_t min_occ, int64_t max_mems, int64_t *mem, int64_t *cnt)
{
	query_begin(h, "smem_dev");
	if (n <= 0) return;
	smem_check("smem_dev", min_len, min_occ, max_mems);
	dev_chunks(n, [&](int64_t i0, int64_t nc) { launch_smem(h, nc, qry, off + i0, 0, min_len, min_occ, max_mems, mem + i0 * max_mems * 5, cnt + i0); });
}

/* ---- sampled suffix array: rows back to (string, position) (k_ssa_build, k_locate) ---- */

static const int64_t SSA_LAUNCH = 1 << 24;                     /* DPP rows (strings, hit slots) per launch: 2^28 threads */

int64_t rb2_hip_ssa_build(rb2_hip_t *h, int log2_step)
{
	query_begin(h, "ssa_build");
	if (log2_step < 0 || log2_step > 30) { rb2_fatal("[rb2_hip] ssa_build: log2_step must be 0 .. 30 (got %d)\n", log2_step); }
	index_rows_change(h);                                      // (an array that is there is freed first: the new one is sized exactly)
	uint64_t N = 0;
	for (int r = 0; r < NR; ++r) N += h->h_rope[r].n;
	const uint64_t n = h->h_rope[0].n;                          // C[1]: rope $ is one piece
	const uint64_t ns = (N + (1ull << log2_step) - 1) >> log2_step;
	if (n) {
		h->ssa_smp.ensure((size_t)ns * 2); h->ssa_len.ensure((size_t)n); h->ssa_head.ensure((size_t)n);
		for (uint64_t k0 = 0; k0 < n; k0 += (uint64_t)SSA_LAUNCH)
			qlaunch(h, k_ssa_build<true>, k_ssa_build<false>, std::min<uint64_t>((uint64_t)SSA_LAUNCH, n - k0), k0, n, log2_step, h->ssa_smp.p, h->ssa_len.p, h->ssa_head.p);
		HIPCHK(hipStreamSynchronize(h->st));
	}
	h->ssa_valid = true; h->ssa_s = log2_step; h->ssa_n = (int64_t)ns; h->ssa_nstr = n;
	return (int64_t)ns;
}

void rb2_hip_ssa_drop(rb2_hip_t *h)
{ finish_pending(h);
	HIPCHK(hipSetDevice(h->dev));
	index_rows_change(h);
}

void rb2_hip_ssa_info(rb2_hip_t *h, int64_t out[4])
{
	out[0] = h->ssa_valid ? 1 : 0; out[1] = h->ssa_s; out[2] = h->ssa_n;
	out[3] = (int64_t)((h->ssa_smp.cap + h->ssa_len.cap + h->ssa_head.cap) * sizeof(uint64_t));
}

static void locate_check(rb2_hip_t *h, const char *who, int64_t max_hits)
{
	if (!h->ssa_valid) { rb2_fatal("[rb2_hip] %s: the index has no sampled suffix array (none was built, or the index changed since): call rb2_hip_ssa_build first\n", who); }
	if (max_hits < 1) { rb2_fatal("[rb2_hip] %s: max_hits must be at least 1 (got %lld)\n", who, (long long)max_hits); }
}

/* n intervals, all device pointers; hit and cnt belong to interval 0 of iv.  One launch takes SSA_LAUNCH slots (split_slots) */
static void launch_locate(rb2_hip_t *h, int64_t n, const int64_t *iv, int64_t max_hits, int64_t *hit, int64_t *cnt)
{
	split_slots(n, max_hits, SSA_LAUNCH, [&](int64_t i0, int64_t nc, int64_t k0, int64_t kc) {
		qlaunch(h, k_locate<true>, k_locate<false>, (uint64_t)(nc * kc), iv + 2 * i0, nc, max_hits, k0, kc, h->ssa_s,
				h->ssa_smp.p, h->ssa_len.p, h->ssa_head.p, h->ssa_nstr, hit + i0 * max_hits * 2, cnt + i0); });
}

int64_t rb2_hip_locate(rb2_hip_t *h, int64_t n, const int64_t *iv, int64_t max_hits, int64_t *hit, int64_t *cnt)
{
	query_begin(h, "locate");
	locate_check(h, "locate", max_hits);
	if (n <= 0) return 0;
	return staged_records(h, n, {nullptr, iv, 2}, 2, max_hits, hit, cnt, [&](int64_t nc, const QStaged &s, int64_t *d_hit, int64_t *d_cnt) {
		launch_locate(h, nc, s.v, max_hits, d_hit, d_cnt); });
}

void rb2_hip_locate_dev(rb2_hip_t *h, int64_t n, const int64_t *iv, int64_t max_hits, int64_t *hit, int64_t *cnt)
{
	query_begin(h, "locate_dev");
	locate_check(h, "locate_dev", max_hits);
	if (n <= 0) return;
	launch_locate(h, n, iv, max_hits, hit, cnt);
}

/* ---- suffix-prefix overlaps: the strings that begin with a suffix of a query (k_overlap, k_string_ids) ---- */

static void launch_overlap(rb2_hip_t *h, int64_t n, const uint8_t *qry, const int64_t *off, int64_t base, int64_t min_ovlp, int64_t max_recs, int64_t *rec, int64_t *cnt)
{
	qlaunch(h, k_overlap<true>, k_overlap<false>, (uint64_t)n, qry, off, base, n, min_ovlp, max_recs, rec, cnt);
}

static void overlap_check(const char *who, int64_t min_ovlp, int64_t max_recs)
{
	if (min_ovlp < 1 || max_recs < 1)
		rb2_fatal("[rb2_hip] %s: min_ovlp and max_recs must be at least 1 (got %lld, %lld)\n", who, (long long)min_ovlp, (long long)max_recs);
}

int64_t rb2_hip_overlap(rb2_hip_t *h, int64_t n, const uint8_t *qry, const int64_t *off, int64_t min_ovlp, int64_t max_recs, int64_t *rec, int64_t *cnt)
{
	query_begin(h, "overlap");
	if (n <= 0) return 0;
	overlap_check("overlap", min_ovlp, max_recs);
	check_offsets("overlap", "query", n, off);
	return staged_records(h, n, {qry, off, 0}, 3, max_recs, rec, cnt, [&](int64_t nc, const QStaged &s, int64_t *d_rec, int64_t *d_cnt) {
		launch_overlap(h, nc, s.bytes, s.v, s.base, min_ovlp, max_recs, d_rec, d_cnt); });
}

void rb2_hip_overlap_dev(rb2_hip_t *h, int64_t n, const uint8_t *qry, const int64_t *off, int64_t min_ovlp, int64_t max_recs, int64_t *rec, int64_t *cnt)
{
	query_begin(h, "overlap_dev");
	if (n <= 0) return;
	overlap_check("overlap_dev", min_ovlp, max_recs);
	dev_chunks(n, [&](int64_t i0, int64_t nc) { launch_overlap(h, nc, qry, off + i0, 0, min_ovlp, max_recs, rec + i0 * max_recs * 3, cnt + i0); });
}

static const int64_t IDS_LAUNCH = 1 << 28;                     /* hit slots (threads) per launch of k_string_ids */

/* n ranges, all device pointers; ids and cnt belong to range 0 of zv.  One launch takes IDS_LAUNCH slots (split_slots), one thread each:
 * k_string_ids reads no rope, so it has no layout and no piece table */
static void launch_string_ids(rb2_hip_t *h, int64_t n, const int64_t *zv, int64_t max_hits, int64_t *ids, int64_t *cnt)
{
	split_slots(n, max_hits, IDS_LAUNCH, [&](int64_t i0, int64_t nc, int64_t k0, int64_t kc) {
		hipLaunchKernelGGL(k_string_ids, dim3((unsigned)cdiv((uint64_t)(nc * kc), 256)), dim3(256), 0, h->st, zv + 2 * i0, (uint64_t)nc, max_hits, k0, kc,
				(const uint64_t*)h->ssa_head.p, h->ssa_nstr, ids + i0 * max_hits, cnt + i0);
		HIPCHK(hipGetLastError()); });
}

int64_t rb2_hip_string_ids(rb2_hip_t *h, int64_t n, const int64_t *zv, int64_t max_hits, int64_t *ids, int64_t *cnt)
{
	query_begin(h, "string_ids");
	locate_check(h, "string_ids", max_hits);
	if (n <= 0) return 0;
	return staged_records(h, n, {nullptr, zv, 2}, 1, max_hits, ids, cnt, [&](int64_t nc, const QStaged &s, int64_t *d_ids, int64_t *d_cnt) {
		launch_string_ids(h, nc, s.v, max_hits, d_ids, d_cnt); });
}

void rb2_hip_string_ids_dev(rb2_hip_t *h, int64_t n, const int64_t *zv, int64_t max_hits, int64_t *ids, int64_t *cnt)
{
	query_begin(h, "string_ids_dev");
	locate_check(h, "string_ids_dev", max_hits);
	if (n <= 0) return;
	launch_string_ids(h, n, zv, max_hits, ids, cnt);
}

/* ---- k-mer enumeration: every k-mer of the indexed strings with its count (k_kmer_expand) ---- */

/* items a frontier segment holds at the most: RB2_KMER_FRONTIER in the environment, read on every call; 2^22 (96 MiB a level, at most
 * 3 GiB at k = 32; a slice of 2^20 items is some hundreds of microseconds of ranks, far above what a launch and its read-back cost) */
static int64_t kmer_frontier() { return std::max(env_i64("RB2_KMER_FRONTIER", (int64_t)1 << 22), KMER_FRONTIER_MIN); }

/* records the staging buffer holds at the most: QUERY_STAGE_BYTES of them; RB2_KMER_STAGE lowers it, to 4 at the least (tests of the flushes) */
static int64_t kmer_stage_limit() { return std::min(std::max<int64_t>(env_i64("RB2_KMER_STAGE", QUERY_STAGE_BYTES / 24), 4), QUERY_STAGE_BYTES / 24); }

int64_t rb2_hip_kmers(rb2_hip_t *h, int k, int64_t min_occ, int canonical, int64_t max_recs, int64_t *rec, int64_t hist_len, int64_t *hist, int64_t info[4])
{
	query_begin(h, "kmers");
	if (k < 1 || k > KMER_MAX_K) { rb2_fatal("[rb2_hip] kmers: k must be 1 .. %d (got %d)\n", KMER_MAX_K, k); }
	if (min_occ < 1) { rb2_fatal("[rb2_hip] kmers: min_occ must be at least 1 (got %lld)\n", (long long)min_occ); }
	if (max_recs < 0 || hist_len < 0) { rb2_fatal("[rb2_hip] kmers: max_recs and hist_len must not be negative (got %lld, %lld)\n", (long long)max_recs, (long long)hist_len); }
	if ((max_recs > 0 && !rec) || (hist_len > 0 && !hist)) { rb2_fatal("[rb2_hip] kmers: %s is NULL but its size is not 0\n", max_recs > 0 && !rec ? "rec" : "hist"); }
	int64_t inf[4] = {0, 0, 0, 0};
	for (int64_t c = 0; c < hist_len; ++c) hist[c] = 0;
	if (info) memcpy(info, inf, sizeof(inf));
	int64_t N = 0;
	for (int r = 0; r < NR; ++r) N += (int64_t)h->h_rope[r].n;
	if (N < min_occ) return 0;                                     // (an empty index: nothing occurs)
	const int64_t F = kmer_frontier(), stage = kmer_stage_recs(max_recs, kmer_stage_limit());
	/* the segments of levels 0 .. k - 1 behind each other in qin, the record staging in qout, three counters and the histogram in qbytes */
	int64_t seg0[KMER_MAX_K + 1], have[KMER_MAX_K] = {0};
	seg0[0] = 0;
	for (int l = 0; l < k; ++l) seg0[l + 1] = seg0[l] + kmer_segment_cap(l, F, N);
	h->qin.ensure((size_t)seg0[k] * 3);
	h->qout.ensure((size_t)std::max<int64_t>(stage, 1) * 3);
	h->qbytes.ensure((size_t)(8 + hist_len) * 8);
	unsigned long long *ctr = (unsigned long long*)h->qbytes.p, *d_hist = ctr + 8;
	HIPCHK(hipMemsetAsync(ctr, 0, (size_t)(8 + hist_len) * 8, h->st));
	const int64_t root[3] = {0, 0, N};
	HIPCHK(hipMemcpyAsync(h->qin.p, root, sizeof(root), hipMemcpyHostToDevice, h->st));
	have[0] = 1; inf[1] = inf[2] = 1;
	int64_t found = 0, flushed = 0;
	auto flush = [&]() {                                           // (the stream is idle: every launch is followed by a synchronise)
		const int64_t m = kmer_staged(found, flushed, max_recs);
		if (m > 0) HIPCHK(hipMemcpyAsync(rec + 3 * flushed, h->qout.p, (size_t)m * 24, hipMemcpyDeviceToHost, h->st));
		flushed += std::max<int64_t>(m, 0);
	};
	int top = 0;
	while (top >= 0) {
		if (have[top] == 0) { --top; continue; }
		const int l = top;
		const bool last = l + 1 == k;
		const int64_t take = last ? kmer_final_slice(have[l], F, stage, max_recs) : kmer_slice(have[l], F);
		have[l] -= take;
		const int64_t *src = h->qin.p + 3 * (seg0[l] + have[l]);      // the slice comes off the end of its segment
		unsigned long long got = 0;
		if (last) {
			if (kmer_must_flush(found, flushed, take, stage, max_recs)) { flush(); HIPCHK(hipStreamSynchronize(h->st)); }
			qlaunch(h, k_kmer_expand<true>, k_kmer_expand<false>, (uint64_t)std::min<int64_t>(take, KMER_ROWS), src, take, l, k, min_occ, canonical ? 1 : 0,
					h->qout.p, stage, flushed, max_recs, ctr, d_hist, hist_len);
			HIPCHK(hipMemcpyAsync(&got, ctr + 1, 8, hipMemcpyDeviceToHost, h->st));
			HIPCHK(hipStreamSynchronize(h->st));
			found = (int64_t)got;
		} else {
			const int64_t cap = seg0[l + 2] - seg0[l + 1];
			HIPCHK(hipMemsetAsync(ctr, 0, 8, h->st));
			qlaunch(h, k_kmer_expand<true>, k_kmer_expand<false>, (uint64_t)std::min<int64_t>(take, KMER_ROWS), src, take, l, k, min_occ, 0,
					h->qin.p + 3 * seg0[l + 1], cap, 0, cap, ctr, d_hist, (int64_t)0);
			HIPCHK(hipMemcpyAsync(&got, ctr, 8, hipMemcpyDeviceToHost, h->st));
			HIPCHK(hipStreamSynchronize(h->st));
			if ((int64_t)got > cap) { rb2_fatal("[rb2_hip] kmers: %llu items for a segment of %lld at level %d (the index is no BWT of strings?)\n", got, (long long)cap, l + 1); }
			have[l + 1] = (int64_t)got;
			inf[1] = std::max(inf[1], have[l + 1]);
			top = l + 1;
			int64_t alive = 0;
			for (int q = 0; q <= top; ++q) alive += have[q] > 0;
			inf[2] = std::max(inf[2], alive);
		}
		++inf[0];
	}
	flush();
	unsigned long long pre = 0;
	HIPCHK(hipMemcpyAsync(&pre, ctr + 2, 8, hipMemcpyDeviceToHost, h->st));
	if (hist_len) HIPCHK(hipMemcpyAsync(hist, d_hist, (size_t)hist_len * 8, hipMemcpyDeviceToHost, h->st));
	HIPCHK(hipStreamSynchronize(h->st));
	inf[3] = (int64_t)pre;
	if (info) memcpy(info, inf, sizeof(inf));
	return found;
}

/* ---- the searches with a step budget ("the path stack"): what rb2_hip_approx, rb2_hip_approx_ed and rb2_hip_irreducible share ---- */

static void budget_check(const char *who, int64_t max_steps, int64_t max_recs)
{
	if (max_steps < 1) { rb2_fatal("[rb2_hip] %s: max_steps must be at least 1 (got %lld)\n", who, (long long)max_steps); }
	if (max_recs < 1) { rb2_fatal("[rb2_hip] %s: max_recs must be at least 1 (got %lld)\n", who, (long long)max_recs); }
}

/* the longest of n queries that is not malformed by its length alone (longer than cap), 1 at the least */
static int64_t longest_wellformed(int64_t n, const int64_t *off, int64_t cap)
{
	int64_t lmax = 1;
	for (int64_t i = 0; i < n; ++i) if (off[i + 1] - off[i] <= cap) lmax = std::max(lmax, off[i + 1] - off[i]);
	return lmax;
}

/* ---- approximate search: the matches of a query within max_mm substitutions (k_approx), or within max_ed edits
 * (k_approx_ed in rb2_edit.h).  A family is its kernel, the stack of a row and the name and the range of its distance ---- */

typedef void (*StackedKernel)(const QTab*, PoolView, const uint8_t*, const int64_t*, int64_t, uint64_t, int, int64_t, int64_t, int64_t, int64_t, int64_t, uint64_t, int64_t, uint8_t*,
                              int64_t*, int64_t*);
struct Stacked { StackedKernel sparse, dense; int64_t (*row_bytes)(int64_t L, int max_dist); const char *dist; int max_dist; };
static const Stacked APPROX = {k_approx<true>, k_approx<false>, [](int64_t L, int) { return approx_row_bytes(L); }, "max_mm", APPROX_MAX_MM};
static const Stacked APPROX_ED = {k_approx_ed<true>, k_approx_ed<false>, [](int64_t L, int max_ed) { return edit_row_bytes(L, max_ed); }, "max_ed", EDIT_MAX_ED};

/* scratch for the stacks of a launch: APPROX_SCRATCH_BYTES; RB2_APPROX_SCRATCH in the environment lowers it (tests of the row cap) */
static int64_t approx_scratch() { return std::min(env_i64("RB2_APPROX_SCRATCH", APPROX_SCRATCH_BYTES), APPROX_SCRATCH_BYTES); }

static void stacked_check(const char *who, const Stacked &f, int dist, int64_t min_occ, int64_t max_steps, int64_t max_recs)
{
	if (dist < 0 || dist > f.max_dist) { rb2_fatal("[rb2_hip] %s: %s must be 0 .. %d (got %d)\n", who, f.dist, f.max_dist, dist); }
	if (min_occ < 1) { rb2_fatal("[rb2_hip] %s: min_occ must be at least 1 (got %lld)\n", who, (long long)min_occ); }
	budget_check(who, max_steps, max_recs);
}

/* n queries, all device pointers, the longest of lmax symbols (APPROX_MAX_LEN when only the device knows): one launch, or one for the
 * short queries and one for the long ones (stack_passes), the stacks sized before the first */
static void launch_stacked(rb2_hip_t *h, const Stacked &f, int64_t n, const uint8_t *qry, const int64_t *off, int64_t base, int64_t lmax, int dist, int64_t min_occ, int64_t max_steps,
                           int64_t max_recs, int64_t *rec, int64_t *cnt)
{
	const auto row_bytes = [&](int64_t L) { return f.row_bytes(L, dist); };
	int64_t pass[2][4], bytes = 0;
	const int np = stack_passes(n, std::min(std::max<int64_t>(lmax, 1), APPROX_MAX_LEN), approx_scratch(), row_bytes, pass);
	for (int k = 0; k < np; ++k) bytes = std::max(bytes, pass[k][3] * row_bytes(pass[k][2]));
	h->qscr.ensure((size_t)bytes);
	for (int k = 0; k < np; ++k)
		qlaunch(h, f.sparse, f.dense, (uint64_t)pass[k][3], qry, off, base, n, dist, min_occ, max_steps, max_recs, pass[k][0], pass[k][1], pass[k][3], pass[k][2], h->qscr.p, rec, cnt);
}

static int64_t stacked_search(rb2_hip_t *h, const Stacked &f, const char *who, int64_t n, const uint8_t *qry, const int64_t *off, int dist, int64_t min_occ, int64_t max_steps,
                              int64_t max_recs, int64_t *rec, int64_t *cnt)
{
	query_begin(h, who);
	if (n <= 0) return 0;
	stacked_check(who, f, dist, min_occ, max_steps, max_recs);
	check_offsets(who, "query", n, off);
	const int64_t lmax = longest_wellformed(n, off, APPROX_MAX_LEN);
	return staged_records(h, n, {qry, off, 0}, 4, max_recs, rec, cnt, [&](int64_t nc, const QStaged &s, int64_t *d_rec, int64_t *d_cnt) {
		launch_stacked(h, f, nc, s.bytes, s.v, s.base, lmax, dist, min_occ, max_steps, max_recs, d_rec, d_cnt); },
		budget_found);                                             // a query that ran out of steps keeps what it had found
}

static void stacked_search_dev(rb2_hip_t *h, const Stacked &f, const char *who, int64_t n, const uint8_t *qry, const int64_t *off, int dist, int64_t min_occ, int64_t max_steps,
                               int64_t max_recs, int64_t *rec, int64_t *cnt)
{
	query_begin(h, who);
	if (n <= 0) return;
	stacked_check(who, f, dist, min_occ, max_steps, max_recs);
	dev_chunks(n, [&](int64_t i0, int64_t nc) {
		launch_stacked(h, f, nc, qry, off + i0, 0, APPROX_MAX_LEN, dist, min_occ, max_steps, max_recs, rec + i0 * max_recs * 4, cnt + i0); });
}

int64_t rb2_hip_approx(rb2_hip_t *h, int64_t n, const uint8_t *qry, const int64_t *off, int max_mm, int64_t min_occ, int64_t max_steps, int64_t max_recs, int64_t *rec, int64_t *cnt)
{
	return stacked_search(h, APPROX, "approx", n, qry, off, max_mm, min_occ, max_steps, max_recs, rec, cnt);
}

void rb2_hip_approx_dev(rb2_hip_t *h, int64_t n, const uint8_t *qry, const int64_t *off, int max_mm, int64_t min_occ, int64_t max_steps, int64_t max_recs, int64_t *rec, int64_t *cnt)
{
	stacked_search_dev(h, APPROX, "approx_dev", n, qry, off, max_mm, min_occ, max_steps, max_recs, rec, cnt);
}

int64_t rb2_hip_approx_ed(rb2_hip_t *h, int64_t n, const uint8_t *qry, const int64_t *off, int max_ed, int64_t min_occ, int64_t max_steps, int64_t max_recs, int64_t *rec, int64_t *cnt)
{
	return stacked_search(h, APPROX_ED, "approx_ed", n, qry, off, max_ed, min_occ, max_steps, max_recs, rec, cnt);
}

void rb2_hip_approx_ed_dev(rb2_hip_t *h, int64_t n, const uint8_t *qry, const int64_t *off, int max_ed, int64_t min_occ, int64_t max_steps, int64_t max_recs, int64_t *rec, int64_t *cnt)
{
	stacked_search_dev(h, APPROX_ED, "approx_ed_dev", n, qry, off, max_ed, min_occ, max_steps, max_recs, rec, cnt);
}

/* ---- duplicate and contained strings: one fused LF walk per string (k_contain) ---- */

/* RB2_CONTAIN_EARLY=0 in the environment, read on every call, makes every walk run to its `$` (tests, and the bench's comparison) */
static int contain_early()
{
	const char *e = getenv("RB2_CONTAIN_EARLY");
	return !(e && strcmp(e, "0") == 0);
}

/* n strings: ids (device memory) or, when ids is NULL, id0 .. id0 + n - 1 */
static void launch_contain(rb2_hip_t *h, int64_t n, const int64_t *ids, int64_t id0, int early, int64_t *rec)
{
	qlaunch(h, k_contain<true>, k_contain<false>, (uint64_t)n, ids, id0, n, early, rec);
}

int64_t rb2_hip_contained(rb2_hip_t *h, int64_t n, const int64_t *ids, int64_t *rec)
{
	query_begin(h, "rb2_hip_contained");
	if (n < 0) { rb2_fatal("[rb2_hip] rb2_hip_contained: the number of ids must not be negative (got %lld)\n", (long long)n); }
	if (n == 0) return 0;
	const int early = contain_early();
	staged_results(h, n, {nullptr, ids, 1}, 5, rec, [&](int64_t nc, const QStaged &s, int64_t *d_rec) { launch_contain(h, nc, s.v, s.base, early, d_rec); });
	int64_t flagged = 0;
	for (int64_t i = 0; i < n; ++i) flagged += rec[5 * i] >= 1 && rec[5 * i] <= 4;
	return flagged;
}

void rb2_hip_contained_dev(rb2_hip_t *h, int64_t n, const int64_t *ids, int64_t *rec)
{
	query_begin(h, "rb2_hip_contained_dev");
	if (n < 0) { rb2_fatal("[rb2_hip] rb2_hip_contained_dev: the number of ids must not be negative (got %lld)\n", (long long)n); }
	const int early = contain_early();
	dev_chunks(n, [&](int64_t i0, int64_t nc) { launch_contain(h, nc, ids ? ids + i0 : nullptr, i0, early, rec + 5 * i0); });
}

/* ---- irreducible overlaps: the neighbours of a read in a string graph (k_irreducible) ---- */

/* scratch for the stacks of a launch: IRRED_SCRATCH_BYTES; RB2_IRRED_SCRATCH in the environment, read on every call, lowers it (tests of the row cap) */
static int64_t irred_scratch() { return std::min(env_i64("RB2_IRRED_SCRATCH", IRRED_SCRATCH_BYTES), IRRED_SCRATCH_BYTES); }

/* n queries, all device pointers, none that counts longer than lmax symbols: one launch, the stacks sized from the entries a row can hold */
static void launch_irreducible(rb2_hip_t *h, int64_t n, const uint8_t *qry, const int64_t *off, int64_t base, int64_t lmax, int64_t min_ovlp, int64_t max_ext,
                               int64_t max_steps, int64_t max_recs, int64_t *rec, int64_t *cnt)
{
	const int64_t cap = irred_entry_cap(lmax, min_ovlp, max_ext, max_steps), row = irred_row_bytes(cap, max_ext), rows = stack_rows(n, row, irred_scratch(), IRRED_ROWS);
	h->qscr.ensure((size_t)(rows * row));
	qlaunch(h, k_irreducible<true>, k_irreducible<false>, (uint64_t)rows, qry, off, base, n, min_ovlp, max_ext, max_steps, max_recs, lmax, rows, cap, h->qscr.p, rec, cnt);
}

static void irreducible_check(const char *who, int64_t max_len, int64_t min_ovlp, int64_t max_ext, int64_t max_steps, int64_t max_recs)
{
	if (min_ovlp < 1) { rb2_fatal("[rb2_hip] %s: min_ovlp must be at least 1 (got %lld)\n", who, (long long)min_ovlp); }
	if (max_ext < 1 || max_ext > IRRED_MAX_LEN) { rb2_fatal("[rb2_hip] %s: max_ext must be 1 .. %lld (got %lld)\n", who, (long long)IRRED_MAX_LEN, (long long)max_ext); }
	budget_check(who, max_steps, max_recs);
	if (max_len < 1 || max_len > IRRED_MAX_LEN) { rb2_fatal("[rb2_hip] %s: max_len must be 1 .. %lld (got %lld)\n", who, (long long)IRRED_MAX_LEN, (long long)max_len); }
}

int64_t rb2_hip_irreducible(rb2_hip_t *h, int64_t n, const uint8_t *qry, const int64_t *off, int64_t min_ovlp, int64_t max_ext, int64_t max_steps, int64_t max_recs,
                            int64_t *rec, int64_t *cnt)
{
	query_begin(h, "irreducible");
	if (n <= 0) return 0;
	irreducible_check("irreducible", 1, min_ovlp, max_ext, max_steps, max_recs);
	check_offsets("irreducible", "query", n, off);
	const int64_t lmax = longest_wellformed(n, off, IRRED_MAX_LEN);
	return staged_records(h, n, {qry, off, 0}, 4, max_recs, rec, cnt, [&](int64_t nc, const QStaged &s, int64_t *d_rec, int64_t *d_cnt) {
		launch_irreducible(h, nc, s.bytes, s.v, s.base, lmax, min_ovlp, max_ext, max_steps, max_recs, d_rec, d_cnt); },
		budget_found);                                             // a query that ran out of steps keeps what it had found
}

void rb2_hip_irreducible_dev(rb2_hip_t *h, int64_t n, const uint8_t *qry, const int64_t *off, int64_t max_len, int64_t min_ovlp, int64_t max_ext, int64_t max_steps,
                             int64_t max_recs, int64_t *rec, int64_t *cnt)
{
	query_begin(h, "irreducible_dev");
	if (n <= 0) return;
	irreducible_check("irreducible_dev", max_len, min_ovlp, max_ext, max_steps, max_recs);
	dev_chunks(n, [&](int64_t i0, int64_t nc) {
		launch_irreducible(h, nc, qry, off + i0, 0, max_len, min_ovlp, max_ext, max_steps, max_recs, rec + i0 * max_recs * 4, cnt + i0); });
}

/* ---- unitigs: the chains of an edge list and their texts (rb2_unitig.h) ---- */

static const int64_t UT_MAX_N = (int64_t)1 << 36;              /* vertices and edges of a call at the most: the scans launch n / 4096 blocks */
static const int64_t UT_LAUNCH = 1 << 24;                      /* DPP rows (vertices) per launch of the pieces' walks: 2^28 threads */

/* one thread per item, the threads striding over what UT_BLOCKS blocks do not cover; nothing for no items */
template <typename... P, typename... A>
static void ulaunch(rb2_hip_t *h, void (*k)(P...), int64_t items, A... a)
{
	if (items <= 0) return;
	hipLaunchKernelGGL(k, dim3((unsigned)std::min<uint64_t>(cdiv((uint64_t)items, 256), UT_BLOCKS)), dim3(256), 0, h->st, static_cast<P>(a)...);
	HIPCHK(hipGetLastError());
}

/* pointer jumps that reach the head of every chain of n vertices: the smallest K with 2^K >= n */
static int unitig_doublings(int64_t n)
{
	int k = 0;
	while (((int64_t)1 << k) < n) ++k;
	return k;
}

struct UtChainBufs { unsigned long long *ctr; uint32_t *outdeg, *indeg; int64_t *inedge, *pred; UtState *st[2]; };

/* the scratch of a chains call, UT_CTRS + 12 n words with the counters and the degrees in front; unitig_chain_bufs: in qscr, those two zeroed */
static UtChainBufs unitig_chain_layout(Carve &c, int64_t n)
{
	UtChainBufs b;
	b.ctr = c.take<unsigned long long>(UT_CTRS);
	b.outdeg = c.take<uint32_t>((size_t)(2 * n)); b.indeg = b.outdeg + n;
	b.inedge = c.take<int64_t>((size_t)(2 * n));
	b.pred = c.take<int64_t>((size_t)n);
	for (int i = 0; i < 2; ++i) b.st[i] = c.take<UtState>((size_t)n);
	return b;
}
static UtChainBufs unitig_chain_bufs(rb2_hip_t *h, int64_t n)
{
	UtChainBufs b;
	carve_in(h->qscr, [&](Carve &c) { b = unitig_chain_layout(c, n); });
	HIPCHK(hipMemsetAsync(b.ctr, 0, (size_t)(UT_CTRS + n) * 8, h->st));
	return b;
}

/* behind the degrees: links, the jumps of the open chains, the cut, the jumps of the cycles, vtx (device memory) */
static void unitig_rank(rb2_hip_t *h, const UtChainBufs &b, int64_t n, int64_t *vtx)
{
	const int K = unitig_doublings(n);
	int cur = 0;
	ulaunch(h, k_unitig_link, n, n, b.outdeg, b.indeg, b.inedge, b.st[0], b.pred, vtx);
	for (int pass = 0; pass < 2; ++pass) {
		for (int k = 0; k < K; ++k, cur ^= 1) ulaunch(h, k_unitig_jump, n, n, b.st[cur], b.st[cur ^ 1]);
		if (pass == 0) { ulaunch(h, k_unitig_cut, n, n, b.st[cur], b.st[cur ^ 1], b.pred, vtx); cur ^= 1; }
	}
	ulaunch(h, k_unitig_fin, n, n, b.st[cur], vtx, b.ctr);
}

static void unitig_chains_check(rb2_hip_t *h, const char *who, int64_t n, int64_t m)
{
	finish_pending(h);
	HIPCHK(hipSetDevice(h->dev));
	if (n < 0 || n > UT_MAX_N || m < 0 || m > UT_MAX_N) { rb2_fatal("[rb2_hip] %s: n_str and m must be 0 .. 2^36 (got %lld, %lld)\n", who, (long long)n, (long long)m); }
}

int64_t rb2_hip_unitig_chains(rb2_hip_t *h, int64_t n_str, int64_t m, const int64_t *edges, int64_t *vtx, int64_t info[4])
{
	unitig_chains_check(h, "unitig_chains", n_str, m);
	const UtChainBufs b = unitig_chain_bufs(h, n_str);
	h->qout.ensure((size_t)(4 * n_str + 4));
	const int64_t CH = query_chunk();
	for (int64_t i0 = 0; i0 < m; i0 += CH) {                       // the edges in chunks: a degree needs no other edge
		const int64_t mc = std::min(CH, m - i0);
		const QStaged s = stage_inputs(h, {nullptr, edges, 4}, i0, mc, 0);
		ulaunch(h, k_unitig_deg, mc, s.v, mc, n_str, b.outdeg, b.indeg, b.inedge, b.ctr);
	}
	unitig_rank(h, b, n_str, h->qout.p);
	int64_t inf[4];
	hipLaunchKernelGGL(k_unitig_info, dim3(1), dim3(64), 0, h->st, (const unsigned long long*)b.ctr, h->qout.p + 4 * n_str);
	HIPCHK(hipGetLastError());
	if (n_str) HIPCHK(hipMemcpyAsync(vtx, h->qout.p, (size_t)n_str * 32, hipMemcpyDeviceToHost, h->st));
	HIPCHK(hipMemcpyAsync(inf, h->qout.p + 4 * n_str, sizeof(inf), hipMemcpyDeviceToHost, h->st));
	HIPCHK(hipStreamSynchronize(h->st));
	if (info) memcpy(info, inf, sizeof(inf));
	return inf[0];
}

void rb2_hip_unitig_chains_dev(rb2_hip_t *h, int64_t n_str, int64_t m, const int64_t *edges, int64_t *vtx, int64_t *info)
{
	unitig_chains_check(h, "unitig_chains_dev", n_str, m);
	const UtChainBufs b = unitig_chain_bufs(h, n_str);
	dev_chunks(m, [&](int64_t i0, int64_t mc) { ulaunch(h, k_unitig_deg, mc, edges + 4 * i0, mc, n_str, b.outdeg, b.indeg, b.inedge, b.ctr); });
	unitig_rank(h, b, n_str, vtx);
	hipLaunchKernelGGL(k_unitig_info, dim3(1), dim3(64), 0, h->st, (const unsigned long long*)b.ctr, info);
	HIPCHK(hipGetLastError());
}

/* exclusive saturating prefix sums of x[0 .. n) in place on the device, their total into *total; bsum: scan_parts(n) words */
static void unitig_scan(rb2_hip_t *h, uint64_t *x, int64_t n, uint64_t *bsum, unsigned long long *total)
{
	scan_launch<ScanSat>(h->st, ScanIn<uint64_t>{x, (uint64_t)n}, (uint64_t)n, bsum, x, (uint64_t*)total, false);
	HIPCHK(hipGetLastError());
}

static void unitig_text_check(rb2_hip_t *h, const char *who, int64_t n, int64_t min_reads, int64_t cap_u, int64_t cap_txt, const void *urec, const void *txt)
{
	query_begin(h, who);
	if (n < 0 || n > UT_MAX_N) { rb2_fatal("[rb2_hip] %s: n_str must be 0 .. 2^36 (got %lld)\n", who, (long long)n); }
	if (min_reads < 1) { rb2_fatal("[rb2_hip] %s: min_reads must be at least 1 (got %lld)\n", who, (long long)min_reads); }
	if (cap_u < 0 || cap_txt < 0) { rb2_fatal("[rb2_hip] %s: cap_u and cap_txt must not be negative (got %lld, %lld)\n", who, (long long)cap_u, (long long)cap_txt); }
	if (cap_u > 0 && cap_txt > 0 && (!urec || !txt)) { rb2_fatal("[rb2_hip] %s: %s is NULL but its size is not 0\n", who, urec ? "txt" : "urec"); }
	if ((uint64_t)n != h->h_rope[0].n) { rb2_fatal("[rb2_hip] %s: n_str = %lld, but the index holds %llu strings\n", who, (long long)n, (unsigned long long)h->h_rope[0].n); }
}

/* vtx, urec and txt in device memory; one synchronise, behind which info is what the counters say.  Returns the chains stored */
static int64_t unitig_text_run(rb2_hip_t *h, int64_t n, const int64_t *vtx, int canonical, int64_t min_reads, int64_t cap_u, int64_t cap_txt, int64_t *urec, uint8_t *txt, int64_t info[4])
{
	int64_t inf[4] = {0, 0, 0, 0};
	if (n > 0) {
		if (cap_u == 0 || cap_txt == 0) cap_u = cap_txt = 0;       // sizes only
		unsigned long long *ctr = nullptr; uint64_t *bsum = nullptr;
		UtHeads H; UtSel S;
		carve_in(h->qscr, [&, N = (size_t)n](Carve &c) {           // UT_CTRS + 10 n + scan_parts(n) words
			ctr = c.take<unsigned long long>(UT_CTRS);
			H.cnt = c.take<unsigned long long>(N);
			H.off = c.take<unsigned long long>(N);
			S.toff = c.take<uint64_t>(N);
			H.flg = (uint32_t*)c.take<uint64_t>(N);                  // (a word each; zeroed up to here)
			H.mn = c.take<unsigned long long>(N);
			H.u = c.take<int64_t>(N);
			S.head = c.take<int64_t>(N);
			S.len = c.take<uint64_t>(N);
			S.tlen = c.take<uint64_t>(N);
			bsum = c.take<uint64_t>(scan_parts((uint64_t)n));
			c.take<uint64_t>(N); });                                 // (n spare words: the buffer has always been this large, nothing uses them)
		HIPCHK(hipMemsetAsync(ctr, 0, (size_t)(UT_CTRS + 4 * n) * 8, h->st));
		HIPCHK(hipMemsetAsync(H.mn, 0xff, (size_t)n * 8, h->st));
		ulaunch(h, k_unitig_sum, n, n, vtx, H);
		ulaunch(h, k_unitig_sel, n, n, H, canonical, min_reads);
		unitig_scan(h, (uint64_t*)H.u, n, bsum, ctr + UT_NSEL);
		ulaunch(h, k_unitig_list, n, n, H, S, canonical, min_reads);
		const uint64_t rows = (uint64_t)std::min<int64_t>(n, UT_ROWS);
		qlaunch(h, k_unitig_len<true>, k_unitig_len<false>, rows, n, ctr, H, S);
		unitig_scan(h, S.toff, n, bsum, ctr + UT_TOTAL);
		if (cap_u) qlaunch(h, k_unitig_text<true, true>, k_unitig_text<false, true>, rows, n, 0, 0, vtx, ctr, H, S, cap_u, cap_txt, txt);
		for (int64_t v0 = 0; v0 < n; v0 += UT_LAUNCH) {              // (always: a short piece shows in the walk, stored or not)
			const int64_t nv = std::min(UT_LAUNCH, n - v0);
			qlaunch(h, k_unitig_text<true, false>, k_unitig_text<false, false>, (uint64_t)nv, n, v0, nv, vtx, ctr, H, S, cap_u, cap_txt, txt);
		}
		ulaunch(h, k_unitig_rec, n, n, ctr, H, S, cap_u, cap_txt, urec);
		unsigned long long c[UT_CTRS];
		HIPCHK(hipMemcpyAsync(c, ctr, sizeof(c), hipMemcpyDeviceToHost, h->st));
		HIPCHK(hipStreamSynchronize(h->st));
		inf[0] = (int64_t)c[UT_NSEL]; inf[1] = (int64_t)c[UT_TOTAL]; inf[2] = (int64_t)c[UT_SHORT]; inf[3] = (int64_t)c[UT_STORED];
	}
	if (info) memcpy(info, inf, sizeof(inf));
	return inf[3];
}

int64_t rb2_hip_unitig_text_dev(rb2_hip_t *h, int64_t n_str, const int64_t *vtx, int canonical, int64_t min_reads, int64_t cap_u, int64_t cap_txt, int64_t *urec, uint8_t *txt,
                                int64_t info[4])
{
	unitig_text_check(h, "unitig_text_dev", n_str, min_reads, cap_u, cap_txt, urec, txt);
	return unitig_text_run(h, n_str, vtx, canonical ? 1 : 0, min_reads, cap_u, cap_txt, urec, txt, info);
}

int64_t rb2_hip_unitig_text(rb2_hip_t *h, int64_t n_str, const int64_t *vtx, int canonical, int64_t min_reads, int64_t cap_u, int64_t cap_txt, int64_t *urec, uint8_t *txt,
                            int64_t info[4])
{
	unitig_text_check(h, "unitig_text", n_str, min_reads, cap_u, cap_txt, urec, txt);
	if (cap_u == 0 || cap_txt == 0) cap_u = cap_txt = 0;
	cap_u = std::min(cap_u, n_str);                                // (no more chains than vertices)
	h->qout.ensure((size_t)(4 * n_str + 5 * cap_u + 1));
	h->qbytes.ensure((size_t)std::max<int64_t>(cap_txt, 1));
	int64_t *d_urec = h->qout.p + 4 * n_str;
	if (n_str) HIPCHK(hipMemcpyAsync(h->qout.p, vtx, (size_t)n_str * 32, hipMemcpyHostToDevice, h->st));
	if (cap_u) HIPCHK(hipMemsetAsync(d_urec, 0xff, (size_t)cap_u * 40, h->st));   // (head -1: a chain that is not stored)
	if (cap_txt) HIPCHK(hipMemsetAsync(h->qbytes.p, 0, (size_t)cap_txt, h->st));  // (what no piece of a damaged vtx covers comes back as 0)
	int64_t inf[4];
	const int64_t stored = unitig_text_run(h, n_str, h->qout.p, canonical ? 1 : 0, min_reads, cap_u, cap_txt, d_urec, h->qbytes.p, inf);
	if (info) memcpy(info, inf, sizeof(inf));
	if (stored > 0) {                                              // only the stored chains reach the caller's buffers: the others' records and slices stay as they were
		std::vector<int64_t> ur((size_t)cap_u * 5);
		const int64_t nu = std::min(cap_u, inf[0]);
		HIPCHK(hipMemcpyAsync(ur.data(), d_urec, (size_t)nu * 40, hipMemcpyDeviceToHost, h->st));
		HIPCHK(hipStreamSynchronize(h->st));
		int64_t lo = -1, hi = -1;                                  // (the slices of stored chains lie behind each other: one copy per run of them)
		auto flush = [&]() { if (hi > lo) HIPCHK(hipMemcpyAsync(txt + lo, h->qbytes.p + lo, (size_t)(hi - lo), hipMemcpyDeviceToHost, h->st)); };
		for (int64_t u = 0; u < nu; ++u) {
			const int64_t *r = ur.data() + 5 * u;
			if (r[0] < 0) continue;
			memcpy(urec + 5 * u, r, 40);
			if (r[2] != hi) { flush(); lo = r[2]; }
			hi = r[2] + r[3];
		}
		flush();
		HIPCHK(hipStreamSynchronize(h->st));
	}
	return stored;
}

/* ---- tip and bubble removal on an edge list (rb2_clean.h) ---- */

static void graph_clean_check(rb2_hip_t *h, const char *who, int64_t n, int64_t m, const int64_t *edges, int64_t max_tip, int64_t max_bubble, int pairs, int64_t max_rounds,
                              int64_t cap, const int64_t *out)
{
	finish_pending(h);
	HIPCHK(hipSetDevice(h->dev));
	if (n < 0 || n > UT_MAX_N || m < 0 || m > UT_MAX_N) { rb2_fatal("[rb2_hip] %s: n_str and m must be 0 .. 2^36 (got %lld, %lld)\n", who, (long long)n, (long long)m); }
	if (max_tip < 0 || max_bubble < 0) { rb2_fatal("[rb2_hip] %s: max_tip_reads and max_bubble_reads must not be negative (got %lld, %lld)\n", who, (long long)max_tip, (long long)max_bubble); }
	if (pairs != 0 && pairs != 1) { rb2_fatal("[rb2_hip] %s: pairs must be 0 or 1 (got %d)\n", who, pairs); }
	if (max_rounds < 1) { rb2_fatal("[rb2_hip] %s: max_rounds must be at least 1 (got %lld)\n", who, (long long)max_rounds); }
	if (cap < 0 || cap > UT_MAX_N) { rb2_fatal("[rb2_hip] %s: cap must be 0 .. 2^36 (got %lld)\n", who, (long long)cap); }
	if (m > 0 && !edges) { rb2_fatal("[rb2_hip] %s: edges is NULL but m is not 0\n", who); }
	if (cap > 0 && !out) { rb2_fatal("[rb2_hip] %s: out is NULL but cap is not 0\n", who); }
	if (m > 0 && cap > 0) {
		const uintptr_t a = (uintptr_t)edges, b = (uintptr_t)out;
		if (a < b + (uintptr_t)cap * 32 && b < a + (uintptr_t)m * 32) { rb2_fatal("[rb2_hip] %s: out overlaps edges\n", who); }
	}
}

/* ed (m rows) and out (cap rows) in device memory, behind graph_clean_check; info = the eight counts.  One synchronise per round (and one
 * more for the chains of the result when the last round allowed still removed rows); the compaction is queued behind the last of them */
static int64_t graph_clean_run(rb2_hip_t *h, int64_t n, int64_t m, const int64_t *ed, int64_t max_tip, int64_t max_bubble, int pairs, int64_t max_rounds, int64_t cap, int64_t *out,
                               int64_t info[8])
{
	const size_t N = (size_t)n, M = (size_t)m, nb = scan_parts((uint64_t)std::max(m, n + 1));
	ClV V;
	unsigned long long *cctr = nullptr; int64_t *vtx = nullptr, *csr = nullptr;
	uint64_t *start = nullptr, *bsum = nullptr; uint32_t *cur = nullptr; uint8_t *dead = nullptr;
	carve_in(h->qscr, [&](Carve &c) {                              // for the whole call: CL_CTRS + 11 n + 1 + m + nb words and m + 3 n bytes ...
		unitig_chain_layout(c, n);                                 // ... behind the room in which unitig_chain_bufs lays out the same again
		cctr = c.take<unsigned long long>(CL_CTRS);
		V.vtx = vtx = c.take<int64_t>(4 * N);
		V.cnt = c.take<unsigned long long>(N);
		V.mn = c.take<unsigned long long>(N);                      // (mn and tail lie together: one memset of 0xff)
		V.tail = c.take<int64_t>(N);
		V.q = c.take<int64_t>(N);
		V.outedge = c.take<int64_t>(N);
		start = c.take<uint64_t>(N + 1);
		csr = c.take<int64_t>(M);                                  // (and, behind the last round, the keep flags and their scan)
		bsum = c.take<uint64_t>(nb);
		V.cls = c.take<uint32_t>(2 * N); cur = V.cls + n;
		dead = c.take<uint8_t>(M + 3 * N); });                     // (dead, lose, a_out, a_in: bytes, no padding between them)
	uint8_t *lose = dead + m, *a_out = lose + n, *a_in = a_out + n;
	if (m) HIPCHK(hipMemsetAsync(dead, 0, (size_t)m, h->st));
	unsigned long long c[CL_CTRS] = {0, 0, 0, 0}, uc[UT_CTRS];
	int64_t rounds = 0, tips = 0, bubbles = 0;
	auto degrees = [&]() -> UtChainBufs {                          // the degrees and the chains of the rows alive
		const UtChainBufs b = unitig_chain_bufs(h, n);
		V.outdeg = b.outdeg; V.indeg = b.indeg; V.inedge = b.inedge;
		HIPCHK(hipMemsetAsync(cctr, 0, CL_CTRS * 8, h->st));
		ulaunch(h, k_clean_deg, m, ed, (const uint8_t*)dead, m, n, b.outdeg, b.indeg, b.inedge, V.outedge, cctr);
		unitig_rank(h, b, n, vtx);
		return b;
	};
	auto counters = [&](const UtChainBufs &b) {
		HIPCHK(hipMemcpyAsync(c, cctr, sizeof(c), hipMemcpyDeviceToHost, h->st));
		HIPCHK(hipMemcpyAsync(uc, b.ctr, sizeof(uc), hipMemcpyDeviceToHost, h->st));
		HIPCHK(hipStreamSynchronize(h->st));
	};
	bool removed = true;
	while (rounds < max_rounds && removed) {
		const UtChainBufs b = degrees();
		if (n) {
			HIPCHK(hipMemsetAsync(V.cnt, 0, (size_t)n * 8, h->st));
			HIPCHK(hipMemsetAsync(V.mn, 0xff, (size_t)n * 16, h->st));
			HIPCHK(hipMemsetAsync(lose, 0, (size_t)n * 3, h->st));
		}
		ulaunch(h, k_clean_sum, n, n, pairs, V);
		ulaunch(h, k_clean_class, n, n, max_tip, V);
		if (max_bubble > 0 && m > 0 && n > 0) {
			ulaunch(h, k_clean_widen, n + 1, n, (const uint32_t*)b.outdeg, start);
			unitig_scan(h, start, n + 1, bsum, cctr + CL_TOTAL);
			HIPCHK(hipMemsetAsync(cur, 0, (size_t)n * 4, h->st));
			ulaunch(h, k_clean_fill, m, ed, (const uint8_t*)dead, m, n, (const uint64_t*)start, cur, csr);
			ulaunch(h, k_clean_rival, n, n, m, max_bubble, V, (const uint64_t*)start, (const int64_t*)csr, lose);
		}
		if (max_tip > 0) ulaunch(h, k_clean_anchor, m, ed, (const uint8_t*)dead, m, n, V, a_out, a_in);
		ulaunch(h, k_clean_mark, m, ed, dead, m, n, V, (const uint8_t*)a_out, (const uint8_t*)a_in, (const uint8_t*)lose, max_tip > 0 ? 1 : 0, max_bubble > 0 ? 1 : 0, cctr);
		counters(b);
		++rounds;
		tips += (int64_t)c[CL_TIPS]; bubbles += (int64_t)c[CL_BUBBLES];
		removed = c[CL_TIPS] + c[CL_BUBBLES] > 0;
	}
	if (removed) counters(degrees());                              // max_rounds cut the loop: the chains of what is left
	const int64_t ignored = (int64_t)c[CL_IGNORED], kept = m - ignored - tips - bubbles, stored = std::min(kept, cap);
	if (kept < 0) { rb2_fatal("[rb2_hip] graph_clean: %lld rows ignored and %lld removed out of %lld\n", (long long)ignored, (long long)(tips + bubbles), (long long)m); }
	if (stored > 0) {
		uint64_t *x = (uint64_t*)csr;
		ulaunch(h, k_clean_keep, m, ed, (const uint8_t*)dead, m, n, x);
		unitig_scan(h, x, m, bsum, cctr + CL_TOTAL);
		ulaunch(h, k_clean_emit, m, ed, (const uint8_t*)dead, m, n, (const uint64_t*)x, cap, out);
	}
	const int64_t inf[8] = {kept, stored, rounds, tips, bubbles, ignored, (int64_t)uc[UT_CHAINS], 0};
	if (info) memcpy(info, inf, sizeof(inf));
	return kept;
}

int64_t rb2_hip_graph_clean_dev(rb2_hip_t *h, int64_t n_str, int64_t m, const int64_t *edges, int64_t max_tip_reads, int64_t max_bubble_reads, int pairs, int64_t max_rounds,
                                int64_t cap, int64_t *out, int64_t info[8])
{
	graph_clean_check(h, "graph_clean_dev", n_str, m, edges, max_tip_reads, max_bubble_reads, pairs, max_rounds, cap, out);
	return graph_clean_run(h, n_str, m, edges, max_tip_reads, max_bubble_reads, pairs, max_rounds, cap, out, info);
}

int64_t rb2_hip_graph_clean(rb2_hip_t *h, int64_t n_str, int64_t m, const int64_t *edges, int64_t max_tip_reads, int64_t max_bubble_reads, int pairs, int64_t max_rounds,
                            int64_t cap, int64_t *out, int64_t info[8])
{
	graph_clean_check(h, "graph_clean", n_str, m, edges, max_tip_reads, max_bubble_reads, pairs, max_rounds, cap, out);
	CallScope cs;
	const int64_t dcap = std::min(cap, m);
	int64_t *rows = scratch<int64_t>(cs, (size_t)(m + dcap) * 4);   // the list and, behind it, the output on the device: no more rows are kept than came
	if (m) HIPCHK(hipMemcpyAsync(rows, edges, (size_t)m * 32, hipMemcpyHostToDevice, h->st));
	int64_t inf[8];
	const int64_t kept = graph_clean_run(h, n_str, m, rows, max_tip_reads, max_bubble_reads, pairs, max_rounds, dcap, dcap ? rows + 4 * m : nullptr, inf);
	inf[1] = std::min(kept, cap);
	if (inf[1] > 0) HIPCHK(hipMemcpyAsync(out, rows + 4 * m, (size_t)inf[1] * 32, hipMemcpyDeviceToHost, h->st));
	HIPCHK(hipStreamSynchronize(h->st));
	if (info) memcpy(info, inf, sizeof(inf));
	return kept;
}

/* ---- the strings of the index, packed, and one index merged into another (rb2_unpack.h, rb2_merge_plan.h) ---- */

static void unpack_check(rb2_hip_t *h, const char *who, int64_t first, int64_t n, int64_t cap)
{
	query_begin(h, who);
	const uint64_t nstr = h->h_rope[0].n;                          // C[1]: rope $ is one piece
	if (first < 0 || n < 0 || (uint64_t)first > nstr || (uint64_t)n > nstr - (uint64_t)first) {
		rb2_fatal("[rb2_hip] %s: strings %lld .. %lld + %lld are no range of the index (it holds %llu)\n", who, (long long)first, (long long)first, (long long)n, (unsigned long long)nstr); }
	if (cap < 0) { rb2_fatal("[rb2_hip] %s: cap must not be negative (got %lld)\n", who, (long long)cap); }
}

/* what the offsets of a range need beside themselves, in qscr: ctr[0] = walks that did not end, ctr[1] = the sum of all; the scan's block sums */
struct UnpackScr { unsigned long long *ctr; uint64_t *bsum; };

/* x[0 .. n] (device) = the offsets of the packed strings first .. first + n - 1: their lengths + 1 by one walk each, x[n] = 0, summed in
 * place.  Queued on the handle's stream */
static UnpackScr unpack_offsets(rb2_hip_t *h, int64_t first, int64_t n, uint64_t *x)
{
	h->qscr.ensure((2 + scan_parts((uint64_t)n + 1)) * 8);
	const UnpackScr s = {(unsigned long long*)h->qscr.p, (uint64_t*)h->qscr.p + 2};
	HIPCHK(hipMemsetAsync(s.ctr, 0, 16, h->st));
	HIPCHK(hipMemsetAsync(x + n, 0, 8, h->st));
	dev_chunks(n, [&](int64_t i0, int64_t nc) { qlaunch(h, k_unpack_len<true>, k_unpack_len<false>, (uint64_t)nc, first + i0, nc, x + i0, s.ctr); });
	unitig_scan(h, x, n + 1, s.bsum, s.ctr + 1);
	return s;
}

/* behind a synchronise: c = the two counters of unpack_offsets.  Returns the sum */
static int64_t unpack_total(const char *who, const unsigned long long c[2])
{
	if (c[0]) { rb2_fatal("[rb2_hip] %s: the walk of a string did not end within the rows of the index (the index is no BWT of complete strings)\n", who); }
	return (int64_t)c[1];
}

/* the texts of strings first .. first + n - 1 into txt[off[i] - base ..), all device pointers, off their n + 1 offsets; queued */
static void unpack_texts(rb2_hip_t *h, int64_t first, int64_t n, const int64_t *off, int64_t base, int reversed, int64_t cap, uint8_t *txt)
{
	dev_chunks(n, [&](int64_t i0, int64_t nc) {
		qlaunch(h, k_unpack_text<true>, k_unpack_text<false>, (uint64_t)nc, first + i0, nc, off + i0, base, reversed ? 1 : 0, cap, txt); });
}

int64_t rb2_hip_unpack_dev(rb2_hip_t *h, int64_t first, int64_t n, int reversed, int64_t cap, uint8_t *txt, int64_t *off)
{
	unpack_check(h, "unpack_dev", first, n, cap);
	if (n == 0) { if (off) HIPCHK(hipMemsetAsync(off, 0, 8, h->st)); return 0; }
	h->qin.ensure((size_t)n + 1);                                   // the offsets are made here: the caller's off is written behind the check of the walks
	uint64_t *x = (uint64_t*)h->qin.p;
	const UnpackScr s = unpack_offsets(h, first, n, x);
	unsigned long long c[2];
	HIPCHK(hipMemcpyAsync(c, s.ctr, sizeof(c), hipMemcpyDeviceToHost, h->st));
	HIPCHK(hipStreamSynchronize(h->st));
	const int64_t size = unpack_total("unpack_dev", c);
	if (off) HIPCHK(hipMemcpyAsync(off, x, (size_t)(n + 1) * 8, hipMemcpyDeviceToDevice, h->st));
	if (txt && cap >= size) unpack_texts(h, first, n, (const int64_t*)x, 0, reversed, size, txt);
	return size;
}

int64_t rb2_hip_unpack(rb2_hip_t *h, int64_t first, int64_t n, int reversed, int64_t cap, uint8_t *txt, int64_t *off)
{
	unpack_check(h, "unpack", first, n, cap);
	if (n == 0) { if (off) off[0] = 0; return 0; }
	const int64_t CH = query_chunk();
	std::vector<int64_t> o((size_t)n + 1);                         // (the caller's off is written behind the check of the walks)
	int64_t run = 0;
	for (int64_t i0 = 0; i0 < n; i0 += CH) {                        // the offsets, chunk by chunk: each chunk's count from 0, the host adds what stands in front
		const int64_t nc = std::min(CH, n - i0);
		h->qin.ensure((size_t)nc + 1);
		const UnpackScr s = unpack_offsets(h, first + i0, nc, (uint64_t*)h->qin.p);
		unsigned long long c[2];
		HIPCHK(hipMemcpyAsync(c, s.ctr, sizeof(c), hipMemcpyDeviceToHost, h->st));
		HIPCHK(hipMemcpyAsync(o.data() + i0, h->qin.p, (size_t)(nc + 1) * 8, hipMemcpyDeviceToHost, h->st));
		HIPCHK(hipStreamSynchronize(h->st));
		unpack_total("unpack", c);
		for (int64_t i = i0; i <= i0 + nc; ++i) o[(size_t)i] += run;
		run = o[(size_t)(i0 + nc)];
	}
	const int64_t size = o[(size_t)n];
	if (off) memcpy(off, o.data(), (size_t)(n + 1) * 8);
	if (!txt || cap < size) return size;
	for (int64_t i0 = 0; i0 < n; ) {                                // the texts: whole strings, at most CH of them and QUERY_STAGE_BYTES of text (one string when it alone is longer)
		const int64_t lim = std::min(n, i0 + CH);
		int64_t i1 = std::upper_bound(o.begin() + i0 + 1, o.begin() + lim + 1, o[(size_t)i0] + QUERY_STAGE_BYTES) - o.begin() - 1;
		i1 = std::max(i1, i0 + 1);
		const int64_t nc = i1 - i0, base = o[(size_t)i0], nb = o[(size_t)i1] - base;
		const QStaged s = stage_inputs(h, {nullptr, o.data(), 1}, i0, nc + 1, 0);
		h->qbytes.ensure((size_t)nb);
		unpack_texts(h, first + i0, nc, s.v, base, reversed, nb, h->qbytes.p);
		HIPCHK(hipMemcpyAsync(txt + base, h->qbytes.p, (size_t)nb, hipMemcpyDeviceToHost, h->st));
		HIPCHK(hipStreamSynchronize(h->st));
		i0 = i1;
	}
	return size;
}

/* the byte budget of a merge's batches and (*max_strings) the strings one may hold: rb2_merge_plan.h says how both follow from the free memory */
static int64_t merge_budget(rb2_hip_t *dst, int64_t batch_bytes, int64_t *max_strings)
{
	int64_t fr = 0, tot = 0;
	rb2_hip_mem_info(dst->dev, &fr, &tot);
	*max_strings = merge_string_cap(fr, (int64_t)max_batch_strings() - 1);
	return batch_bytes > 0 ? batch_bytes : env_i64("RB2_MERGE_BATCH", merge_default_budget(fr));
}

/* All n (>= 1) strings of src as one batch text, cut into the batches that dst takes (rb2_hip_merge, rb2_hip_correct_into).  x = their
 * offsets, which stay on the device (8 bytes a string, in src's staging buffer); the host gets the block sums of the scan that made them
 * (bsum[b] = off[b * B]: rb2_scan.h) and, per batch, the offsets of one block.  One synchronise of src's stream here and one per cut */
struct BatchSource {
	rb2_hip_t *src;
	int64_t n, nb, total, budget, max_strings;
	uint64_t *x;
	std::vector<uint64_t> bsum, blk;
	BatchSource(rb2_hip_t *dst, rb2_hip_t *src_, const char *who, int64_t n_, int64_t batch_bytes)
		: src(src_), n(n_), nb((int64_t)cdiv((uint64_t)n_, SCAN_ITEMS)), bsum((size_t)nb), blk((size_t)SCAN_ITEMS)
	{
		src->qin.ensure((size_t)n + 1);
		x = (uint64_t*)src->qin.p;
		const UnpackScr s = unpack_offsets(src, 0, n, x);
		unsigned long long c[2];
		HIPCHK(hipMemcpyAsync(c, s.ctr, sizeof(c), hipMemcpyDeviceToHost, src->st));
		HIPCHK(hipMemcpyAsync(bsum.data(), s.bsum, (size_t)nb * 8, hipMemcpyDeviceToHost, src->st));
		HIPCHK(hipStreamSynchronize(src->st));
		total = unpack_total(who, c);
		budget = merge_budget(dst, batch_bytes, &max_strings);
	}
	/* the batch that begins with string i0, whose offset is off0 (merge_next_cut) */
	MergeCut next_cut(int64_t i0, int64_t off0)
	{
		const int64_t B = SCAN_ITEMS;
		return merge_next_cut(bsum.data(), nb, n, (uint64_t)total, B, i0, (uint64_t)off0, (uint64_t)budget, max_strings, blk.data(), [&](int64_t b, uint64_t *buf) {
			HIPCHK(hipMemcpyAsync(buf, x + b * B, (size_t)std::min(B, n - b * B) * 8, hipMemcpyDeviceToHost, src->st));
			HIPCHK(hipStreamSynchronize(src->st)); });
	}
};

int64_t rb2_hip_merge(rb2_hip_t *dst, rb2_hip_t *src, int64_t batch_bytes, int64_t info[4])
{
	if (!dst || !src || dst == src) { rb2_fatal("[rb2_hip] merge: dst and src must be two different handles\n"); }
	if (dst->dev != src->dev) { rb2_fatal("[rb2_hip] merge: dst is on device %d and src on device %d; both indexes must be on one device\n", dst->dev, src->dev); }
	if (dst->nranks > 1 || src->nranks > 1) { rb2_fatal("[rb2_hip] merge: %s holds only its own sub-ropes of a sharded index; a merge needs both indexes whole, each on one engine\n", dst->nranks > 1 ? "dst" : "src"); }
	if (batch_bytes < 0) { rb2_fatal("[rb2_hip] merge: batch_bytes must not be negative (got %lld)\n", (long long)batch_bytes); }
	finish_pending(dst);
	query_begin(src, "merge");
	int64_t inf[4] = {0, 0, 0, 0};
	if (info) memcpy(info, inf, sizeof(inf));
	const int64_t n = (int64_t)src->h_rope[0].n;
	if (n == 0) return 0;
	BatchSource S(dst, src, "merge", n, batch_bytes);
	const int64_t total = S.total;
	HIPCHK(hipSetDevice(dst->dev));
	CallScope cs;
	auto &text = cs.make<DevBuf<uint8_t>>();
	text.ensure((size_t)std::min(S.budget, total) + 64);
	int64_t i0 = 0, off0 = 0;
	while (i0 < n) {
		const MergeCut cut = S.next_cut(i0, off0);
		const int64_t len = (int64_t)cut.off_end - off0;
		text.ensure((size_t)len + 64);                              // (grows for a string longer than the budget only)
		unpack_texts(src, i0, cut.end - i0, (const int64_t*)S.x + i0, off0, 1, len, text.p);
		HIPCHK(hipStreamSynchronize(src->st));                      // the two handles have streams of their own: the batch is complete before dst reads it ...
		rb2_hip_insert_multi_dev(dst, len, text.p);
		HIPCHK(hipStreamSynchronize(dst->st));                      // ... and read before src writes the next one
		++inf[2]; inf[3] = std::max(inf[3], len);
		i0 = cut.end; off0 = (int64_t)cut.off_end;
	}
	inf[0] = n; inf[1] = total - n;
	if (info) memcpy(info, inf, sizeof(inf));
	return total;
}

/* ---- the string graph of the index's own strings (rb2_graph.h, rb2_graph_plan.h) ---- */

/* strings of a chunk at the most: RB2_GRAPH_CHUNK in the environment, read on every call; RB2_QUERY_CHUNK's limit otherwise and at the most */
static int64_t graph_chunk() { return std::min<int64_t>(env_i64("RB2_GRAPH_CHUNK", 1 << 24), 1 << 24); }

static void string_graph_check(rb2_hip_t *h, const char *who, int64_t first, int64_t n, int64_t min_ovlp, int64_t max_ext, int64_t max_steps, int64_t max_recs, int64_t max_hits,
                               int pairs, int64_t cap, const int64_t *edges)
{
	finish_pending(h);
	const uint64_t nstr = h->h_rope[0].n;                          // C[1]: rope $ is one piece
	if (h->nranks > 1) rb2_fatal("[rb2_hip] %s: this handle holds only its own sub-ropes of a sharded index; queries need the whole index on one engine\n", who);
	if (!h->ssa_valid) { rb2_fatal("[rb2_hip] %s: the index has no sampled suffix array (none was built, or the index changed since): call rb2_hip_ssa_build first\n", who); }
	if (first < 0 || n < 0 || (uint64_t)first > nstr || (uint64_t)n > nstr - (uint64_t)first) {
		rb2_fatal("[rb2_hip] %s: strings %lld .. %lld + %lld are no range of the index (it holds %llu)\n", who, (long long)first, (long long)first, (long long)n, (unsigned long long)nstr); }
	if (cap < 0) { rb2_fatal("[rb2_hip] %s: cap must not be negative (got %lld)\n", who, (long long)cap); }
	if (cap > 0 && !edges) { rb2_fatal("[rb2_hip] %s: edges is NULL but cap is not 0\n", who); }
	irreducible_check(who, 1, min_ovlp, max_ext, max_steps, max_recs);
	if (max_hits < 1) { rb2_fatal("[rb2_hip] %s: max_hits must be at least 1 (got %lld)\n", who, (long long)max_hits); }
	if (pairs && nstr % 2) { rb2_fatal("[rb2_hip] %s: pairs needs strings 2i and 2i + 1 to be the two strands of a read, but the index holds %llu strings\n", who, (unsigned long long)nstr); }
}

/* edges (cap rows) in device memory, behind string_graph_check; info = the eight counts.  One synchronise per chunk and one at the end */
static int64_t string_graph_run(rb2_hip_t *h, const char *who, int64_t first, int64_t n, int64_t min_ovlp, int64_t max_ext, int64_t max_steps, int64_t max_recs, int64_t max_hits,
                                int pairs, int64_t cap, int64_t *edges, int64_t info[8])
{
	int64_t inf[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	if (info) memcpy(info, inf, sizeof(inf));
	if (n == 0) return 0;
	query_begin(h, who);
	GraphPlan plan = graph_plan(graph_chunk(), max_recs);
	/* qin for the whole call, so that it never moves: the offsets of a chunk, its cnt, its edge counts, their block sums, the words of the call */
	const int64_t most = std::min(plan.limit, n), nbs = (int64_t)scan_parts((uint64_t)most + 1);
	uint64_t *x = nullptr, *e = nullptr, *bsum = nullptr; int64_t *cnt = nullptr; unsigned long long *gc = nullptr;
	carve_in(h->qin, [&](Carve &c) {                               // 3 most + 2 + nbs + GR_WORDS words
		x = c.take<uint64_t>((size_t)most + 1); e = c.take<uint64_t>((size_t)most + 1);
		bsum = c.take<uint64_t>((size_t)nbs);
		cnt = c.take<int64_t>((size_t)most);
		gc = c.take<unsigned long long>(GR_WORDS); });
	HIPCHK(hipMemsetAsync(gc, 0, GR_WORDS * 8, h->st));
	for (int64_t i0 = 0; i0 < n; ) {
		const int64_t tried = graph_try(plan, n - i0);
		const UnpackScr s = unpack_offsets(h, first + i0, tried, x);
		hipLaunchKernelGGL(k_graph_cut, dim3(1), dim3(1), 0, h->st, (const uint64_t*)x, (uint64_t)tried, (uint64_t)GRAPH_TEXT_BYTES, gc);
		ulaunch(h, k_graph_lmax, tried, (const uint64_t*)x, gc);
		unsigned long long c[2], g[3];
		HIPCHK(hipMemcpyAsync(c, s.ctr, sizeof(c), hipMemcpyDeviceToHost, h->st));
		HIPCHK(hipMemcpyAsync(g, gc, sizeof(g), hipMemcpyDeviceToHost, h->st));
		HIPCHK(hipStreamSynchronize(h->st));
		unpack_total(who, c);
		const int64_t nc = (int64_t)g[GR_TOOK], nb = (int64_t)g[GR_BYTES];
		const int64_t lmax = std::min(std::max<int64_t>((int64_t)g[GR_LMAX] - 1, 1), IRRED_MAX_LEN);
		if (nc < 1 || nc > tried) { rb2_fatal("[rb2_hip] %s: a chunk of %lld strings out of %lld tried\n", who, (long long)nc, (long long)tried); }
		h->qbytes.ensure((size_t)std::max<int64_t>(nb, 1));
		h->qout.ensure((size_t)(nc * max_recs) * 4);
		unpack_texts(h, first + i0, nc, (const int64_t*)x, 0, 0, nb, h->qbytes.p);
		{
			const int64_t ecap = irred_entry_cap(lmax, min_ovlp, max_ext, max_steps), row = irred_row_bytes(ecap, max_ext), rows = stack_rows(nc, row, irred_scratch(), IRRED_ROWS);
			h->qscr.ensure((size_t)(rows * row));
			qlaunch(h, k_irreducible<true, true>, k_irreducible<false, true>, (uint64_t)rows, (const uint8_t*)h->qbytes.p, (const int64_t*)x, 0, nc, min_ovlp, max_ext, max_steps, max_recs, lmax,
					rows, ecap, h->qscr.p, h->qout.p, cnt);
		}
		ulaunch(h, k_graph_count, nc, nc, (const int64_t*)x, (const int64_t*)h->qout.p, (const int64_t*)cnt, max_recs, max_hits, e, gc);
		HIPCHK(hipMemsetAsync(e + nc, 0, 8, h->st));
		unitig_scan(h, e, nc + 1, bsum, gc + GR_CHUNK);
		hipLaunchKernelGGL(k_graph_emit, dim3((unsigned)cdiv((uint64_t)nc, QPB)), dim3(256), 0, h->st, (uint64_t)nc, first + i0, (const int64_t*)h->qout.p, (const int64_t*)cnt, (const uint64_t*)e,
				max_recs, max_hits, pairs ? 1 : 0, (const uint64_t*)h->ssa_head.p, h->ssa_nstr, (const unsigned long long*)gc, (uint64_t)cap, edges);
		HIPCHK(hipGetLastError());
		graph_took(plan, tried, nc);
		i0 += nc;
	}
	unsigned long long g[GR_WORDS];
	HIPCHK(hipMemcpyAsync(g, gc, sizeof(g), hipMemcpyDeviceToHost, h->st));
	HIPCHK(hipStreamSynchronize(h->st));
	inf[0] = (int64_t)std::min<unsigned long long>(g[GR_BASE] + g[GR_CHUNK], UT_SAT);
	inf[1] = std::min(inf[0], cap);
	inf[2] = (int64_t)g[GR_OVER_RECS]; inf[3] = (int64_t)g[GR_OVER_HITS]; inf[4] = (int64_t)g[GR_OVER_STEPS]; inf[5] = (int64_t)g[GR_TOO_LONG];
	if (info) memcpy(info, inf, sizeof(inf));
	return inf[0];
}

int64_t rb2_hip_string_graph_dev(rb2_hip_t *h, int64_t first, int64_t n, int64_t min_ovlp, int64_t max_ext, int64_t max_steps, int64_t max_recs, int64_t max_hits, int pairs,
                                 int64_t cap, int64_t *edges, int64_t info[8])
{
	string_graph_check(h, "string_graph_dev", first, n, min_ovlp, max_ext, max_steps, max_recs, max_hits, pairs, cap, edges);
	return string_graph_run(h, "string_graph_dev", first, n, min_ovlp, max_ext, max_steps, max_recs, max_hits, pairs, cap, edges, info);
}

int64_t rb2_hip_string_graph(rb2_hip_t *h, int64_t first, int64_t n, int64_t min_ovlp, int64_t max_ext, int64_t max_steps, int64_t max_recs, int64_t max_hits, int pairs,
                             int64_t cap, int64_t *edges, int64_t info[8])
{
	string_graph_check(h, "string_graph", first, n, min_ovlp, max_ext, max_steps, max_recs, max_hits, pairs, cap, edges);
	HIPCHK(hipSetDevice(h->dev));
	CallScope cs;
	int64_t *rows = scratch<int64_t>(cs, n > 0 ? (size_t)cap * 4 : 0);   // the output on the device: cap rows, of which min(m, cap) come back
	int64_t inf[8];
	const int64_t m = string_graph_run(h, "string_graph", first, n, min_ovlp, max_ext, max_steps, max_recs, max_hits, pairs, cap, rows, inf);
	if (inf[1] > 0) {
		HIPCHK(hipMemcpyAsync(edges, rows, (size_t)inf[1] * 32, hipMemcpyDeviceToHost, h->st));
		HIPCHK(hipStreamSynchronize(h->st));
	}
	if (info) memcpy(info, inf, sizeof(inf));
	return m;
}

/* ---- reads corrected by the k-mer spectrum of the index (k_correct in rb2_correct.h, the rule in rb2_correct_plan.h) ---- */

/* rows of a launch at the most: CORRECT_ROWS; RB2_CORRECT_ROWS in the environment, read on every call, lowers it (tests of rows that take several reads) */
static int64_t correct_row_cap() { return std::min(env_i64("RB2_CORRECT_ROWS", CORRECT_ROWS), CORRECT_ROWS); }

static void correct_check(const char *who, int64_t k, int64_t min_occ, int64_t max_fix, int64_t max_probes)
{
	if (k < 1) { rb2_fatal("[rb2_hip] %s: k must be at least 1 (got %lld)\n", who, (long long)k); }
	if (min_occ < 1) { rb2_fatal("[rb2_hip] %s: min_occ must be at least 1 (got %lld)\n", who, (long long)min_occ); }
	if (max_fix < 1) { rb2_fatal("[rb2_hip] %s: max_fix must be at least 1 (got %lld)\n", who, (long long)max_fix); }
	if (max_probes < 1) { rb2_fatal("[rb2_hip] %s: max_probes must be at least 1 (got %lld)\n", who, (long long)max_probes); }
}

/* n items, all device pointers: item i is string i * stride of the packed batch (end0: packed strings with their closing 0); one launch,
 * the solid bits in LDS, so nothing is sized here */
static void launch_correct(rb2_hip_t *h, int64_t n, int64_t stride, bool end0, const uint8_t *qry, const int64_t *off, int64_t base, int64_t k, int64_t min_occ, int64_t max_fix,
                           int64_t max_probes, uint8_t *out, int64_t *cnt, int64_t *weak)
{
	const int64_t rows = correct_rows(n, correct_row_cap());
	if (end0) qlaunch(h, k_correct<true, true>, k_correct<false, true>, (uint64_t)rows, qry, off, base, n, stride, k, min_occ, max_fix, max_probes, rows, out, cnt, weak);
	else qlaunch(h, k_correct<true, false>, k_correct<false, false>, (uint64_t)rows, qry, off, base, n, stride, k, min_occ, max_fix, max_probes, rows, out, cnt, weak);
}

int64_t rb2_hip_correct(rb2_hip_t *h, int64_t n, const uint8_t *qry, const int64_t *off, int64_t k, int64_t min_occ, int64_t max_fix, int64_t max_probes, uint8_t *out, int64_t *cnt, int64_t *weak)
{
	query_begin(h, "correct");
	if (n <= 0) return 0;
	correct_check("correct", k, min_occ, max_fix, max_probes);
	check_offsets("correct", "read", n, off);
	const int64_t CH = query_chunk();
	int64_t fixes = 0;
	for (int64_t i0 = 0; i0 < n; i0 += CH) {                        // the text of a chunk comes back as it went: the same bytes of out
		const int64_t nc = std::min(CH, n - i0), nb = off[i0 + nc] - off[i0];
		const QStaged s = stage_inputs(h, {qry, off, 0}, i0, nc, 2 * nc);
		h->qout.ensure((size_t)nb / 8 + 1);
		launch_correct(h, nc, 1, false, s.bytes, s.v, s.base, k, min_occ, max_fix, max_probes, (uint8_t*)h->qout.p, s.tail, s.tail + nc);
		HIPCHK(hipMemcpyAsync(cnt + i0, s.tail, (size_t)nc * 8, hipMemcpyDeviceToHost, h->st));
		HIPCHK(hipMemcpyAsync(weak + i0, s.tail + nc, (size_t)nc * 8, hipMemcpyDeviceToHost, h->st));
		if (nb) HIPCHK(hipMemcpyAsync(out + s.base, h->qout.p, (size_t)nb, hipMemcpyDeviceToHost, h->st));
		HIPCHK(hipStreamSynchronize(h->st));
		for (int64_t i = i0; i < i0 + nc; ++i) fixes += budget_found(cnt[i]);
	}
	return fixes;
}

void rb2_hip_correct_dev(rb2_hip_t *h, int64_t n, const uint8_t *qry, const int64_t *off, int64_t total, int64_t k, int64_t min_occ, int64_t max_fix, int64_t max_probes,
                         uint8_t *out, int64_t *cnt, int64_t *weak)
{
	query_begin(h, "correct_dev");
	if (n <= 0) return;
	correct_check("correct_dev", k, min_occ, max_fix, max_probes);
	if (total < 0) { rb2_fatal("[rb2_hip] correct_dev: total must not be negative (got %lld)\n", (long long)total); }
	dev_chunks(n, [&](int64_t i0, int64_t nc) { launch_correct(h, nc, 1, false, qry, off + i0, 0, k, min_occ, max_fix, max_probes, out, cnt + i0, weak + i0); });
}

int64_t rb2_hip_correct_into(rb2_hip_t *dst, rb2_hip_t *src, int64_t k, int64_t min_occ, int64_t max_fix, int64_t max_probes, int pairs, int64_t batch_bytes, int64_t info[8])
{
	if (!dst || !src || dst == src) { rb2_fatal("[rb2_hip] correct_into: dst and src must be two different handles\n"); }
	if (dst->dev != src->dev) { rb2_fatal("[rb2_hip] correct_into: dst is on device %d and src on device %d; both indexes must be on one device\n", dst->dev, src->dev); }
	if (dst->nranks > 1 || src->nranks > 1) { rb2_fatal("[rb2_hip] correct_into: %s holds only its own sub-ropes of a sharded index; the call needs both indexes whole, each on one engine\n", dst->nranks > 1 ? "dst" : "src"); }
	if (batch_bytes < 0) { rb2_fatal("[rb2_hip] correct_into: batch_bytes must not be negative (got %lld)\n", (long long)batch_bytes); }
	correct_check("correct_into", k, min_occ, max_fix, max_probes);
	finish_pending(dst);
	query_begin(src, "correct_into");
	int64_t inf[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	if (info) memcpy(info, inf, sizeof(inf));
	const int64_t n = (int64_t)src->h_rope[0].n;
	if (pairs && n % 2) { rb2_fatal("[rb2_hip] correct_into: pairs needs strings 2i and 2i + 1 to be the two strands of a read, but src holds %lld strings\n", (long long)n); }
	if (n == 0) return 0;
	const int64_t stride = pairs ? 2 : 1;
	BatchSource S(dst, src, "correct_into", n, batch_bytes);
	const int64_t total = S.total, budget = S.budget;
	const uint64_t *x = S.x;
	unsigned long long cc[CORRECT_CTRS];
	HIPCHK(hipSetDevice(dst->dev));
	CallScope cs;
	auto &text = cs.make<DevBuf<uint8_t>>(), &batch = cs.make<DevBuf<uint8_t>>();   // a batch as it was unpacked (text order), and what becomes the insert batch
	auto &res = cs.make<DevBuf<int64_t>>();                         // the counters of the call, then cnt and weak of a batch
	text.ensure((size_t)std::min(budget, total) + 64);
	batch.ensure((size_t)std::min(budget, total) + 64);
	res.ensure((size_t)CORRECT_CTRS);
	HIPCHK(hipMemsetAsync(res.p, 0, CORRECT_CTRS * 8, src->st));
	int64_t i0 = 0, off0 = 0;
	while (i0 < n) {
		MergeCut cut = S.next_cut(i0, off0);
		if (pairs && (cut.end - i0) % 2) {                          // whole pairs: one string less, or the pair when its first string alone is a batch
			cut.end += cut.end - i0 == 1 ? 1 : -1;
			HIPCHK(hipMemcpyAsync(&cut.off_end, x + cut.end, 8, hipMemcpyDeviceToHost, src->st));
			HIPCHK(hipStreamSynchronize(src->st));
		}
		const int64_t len = (int64_t)cut.off_end - off0, ns = cut.end - i0, items = ns / stride;
		text.ensure((size_t)len + 64);                              // (these grow for a string longer than the budget only)
		batch.ensure((size_t)len + 64);
		res.ensure((size_t)(CORRECT_CTRS + 2 * items), true, src->st);   // (the counters move with the array)
		int64_t *cnt = res.p + CORRECT_CTRS, *weak = cnt + items;
		const int64_t *o = (const int64_t*)x + i0;
		unpack_texts(src, i0, ns, o, off0, 0, len, text.p);
		launch_correct(src, items, stride, true, text.p, o, off0, k, min_occ, max_fix, max_probes, batch.p, cnt, weak);
		hipLaunchKernelGGL(k_correct_mate, dim3((unsigned)cdiv((uint64_t)items, QPB)), dim3(256), 0, src->st, (uint64_t)items, (uint64_t)stride, (const uint8_t*)text.p, batch.p, o, off0,
				(const int64_t*)cnt, (const int64_t*)weak, (unsigned long long*)res.p);
		hipLaunchKernelGGL(k_correct_reverse, dim3((unsigned)cdiv((uint64_t)items, QPB)), dim3(256), 0, src->st, (uint64_t)items, (uint64_t)stride, batch.p, o, off0);
		HIPCHK(hipGetLastError());
		HIPCHK(hipStreamSynchronize(src->st));                      // the two handles have streams of their own: the batch is complete before dst reads it ...
		rb2_hip_insert_multi_dev(dst, len, batch.p);
		HIPCHK(hipStreamSynchronize(dst->st));                      // ... and read before src writes the next one
		++inf[6]; inf[7] = std::max(inf[7], len);
		i0 = cut.end; off0 = (int64_t)cut.off_end;
	}
	HIPCHK(hipMemcpyAsync(cc, res.p, sizeof(cc), hipMemcpyDeviceToHost, src->st));
	HIPCHK(hipStreamSynchronize(src->st));
	inf[0] = n; inf[1] = (int64_t)cc[CC_CHANGED]; inf[2] = (int64_t)cc[CC_FIXES]; inf[3] = (int64_t)cc[CC_WEAK]; inf[4] = (int64_t)cc[CC_OVER]; inf[5] = (int64_t)cc[CC_BAD];
	if (info) memcpy(info, inf, sizeof(inf));
	return total;
}
