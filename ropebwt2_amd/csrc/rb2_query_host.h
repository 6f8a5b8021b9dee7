// Host side of the FM-index queries (kernels: rb2_query.h; the launch arithmetic: rb2_query_plan.h, rb2_kmer_plan.h).  Included from rb2_engine.hip, whose
// handle, buffers and checks it uses.  Four helpers carry every query: qlaunch (one launch of a kernel in the layout of the index),
// stage_inputs (a chunk's inputs to the device), staged_records (the chunked loop of the host variants that return records) and
// dev_chunks (the chunked loop of the device-pointer variants).
#pragma once
#include "rb2_query_plan.h"
#include "rb2_kmer_plan.h"

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
static int64_t kmer_frontier()
{
	const char *e = getenv("RB2_KMER_FRONTIER");
	const int64_t v = e ? atoll(e) : 0;
	return v > 0 ? std::max(v, KMER_FRONTIER_MIN) : (int64_t)1 << 22;
}

/* records the staging buffer holds at the most: QUERY_STAGE_BYTES of them; RB2_KMER_STAGE lowers it (tests of the flushes) */
static int64_t kmer_stage_limit()
{
	const int64_t lim = QUERY_STAGE_BYTES / 24;
	const char *e = getenv("RB2_KMER_STAGE");
	const int64_t v = e ? atoll(e) : 0;
	return v > 0 ? std::min(std::max<int64_t>(v, 4), lim) : lim;
}

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

/* ---- approximate search: the matches of a query within max_mm substitutions (k_approx) ---- */

/* scratch for the stacks of a launch: APPROX_SCRATCH_BYTES; RB2_APPROX_SCRATCH in the environment lowers it (tests of the row cap) */
static int64_t approx_scratch()
{
	const char *e = getenv("RB2_APPROX_SCRATCH");
	const int64_t v = e ? atoll(e) : 0;
	return v > 0 ? std::min(v, APPROX_SCRATCH_BYTES) : APPROX_SCRATCH_BYTES;
}

/* n queries, all device pointers, the longest of lmax symbols (APPROX_MAX_LEN when only the device knows): one launch, or one for the
 * short queries and one for the long ones (approx_passes), the stacks sized before the first */
static void launch_approx(rb2_hip_t *h, int64_t n, const uint8_t *qry, const int64_t *off, int64_t base, int64_t lmax, int max_mm, int64_t min_occ, int64_t max_steps,
                          int64_t max_recs, int64_t *rec, int64_t *cnt)
{
	int64_t pass[2][4], bytes = 0;
	const int np = approx_passes(n, std::min(std::max<int64_t>(lmax, 1), APPROX_MAX_LEN), approx_scratch(), pass);
	for (int k = 0; k < np; ++k) bytes = std::max(bytes, pass[k][3] * approx_row_bytes(pass[k][2]));
	h->qscr.ensure((size_t)bytes);
	for (int k = 0; k < np; ++k)
		qlaunch(h, k_approx<true>, k_approx<false>, (uint64_t)pass[k][3], qry, off, base, n, max_mm, min_occ, max_steps, max_recs, pass[k][0], pass[k][1],
				pass[k][3], pass[k][2], h->qscr.p, rec, cnt);
}

static void approx_check(const char *who, int max_mm, int64_t min_occ, int64_t max_steps, int64_t max_recs)
{
	if (max_mm < 0 || max_mm > APPROX_MAX_MM) { rb2_fatal("[rb2_hip] %s: max_mm must be 0 .. %d (got %d)\n", who, APPROX_MAX_MM, max_mm); }
	if (min_occ < 1) { rb2_fatal("[rb2_hip] %s: min_occ must be at least 1 (got %lld)\n", who, (long long)min_occ); }
	if (max_steps < 1) { rb2_fatal("[rb2_hip] %s: max_steps must be at least 1 (got %lld)\n", who, (long long)max_steps); }
	if (max_recs < 1) { rb2_fatal("[rb2_hip] %s: max_recs must be at least 1 (got %lld)\n", who, (long long)max_recs); }
}

int64_t rb2_hip_approx(rb2_hip_t *h, int64_t n, const uint8_t *qry, const int64_t *off, int max_mm, int64_t min_occ, int64_t max_steps, int64_t max_recs, int64_t *rec, int64_t *cnt)
{
	query_begin(h, "approx");
	if (n <= 0) return 0;
	approx_check("approx", max_mm, min_occ, max_steps, max_recs);
	check_offsets("approx", "query", n, off);
	int64_t lmax = 1;                                              // the longest query that is not malformed by its length alone
	for (int64_t i = 0; i < n; ++i) if (off[i + 1] - off[i] <= APPROX_MAX_LEN) lmax = std::max(lmax, off[i + 1] - off[i]);
	return staged_records(h, n, {qry, off, 0}, 4, max_recs, rec, cnt, [&](int64_t nc, const QStaged &s, int64_t *d_rec, int64_t *d_cnt) {
		launch_approx(h, nc, s.bytes, s.v, s.base, lmax, max_mm, min_occ, max_steps, max_recs, d_rec, d_cnt); },
		[](int64_t c) { return c >= 0 ? c : c <= -2 ? -2 - c : 0; });     // a query that ran out of steps keeps what it had found
}

void rb2_hip_approx_dev(rb2_hip_t *h, int64_t n, const uint8_t *qry, const int64_t *off, int max_mm, int64_t min_occ, int64_t max_steps, int64_t max_recs, int64_t *rec, int64_t *cnt)
{
	query_begin(h, "approx_dev");
	if (n <= 0) return;
	approx_check("approx_dev", max_mm, min_occ, max_steps, max_recs);
	dev_chunks(n, [&](int64_t i0, int64_t nc) {
		launch_approx(h, nc, qry, off + i0, 0, APPROX_MAX_LEN, max_mm, min_occ, max_steps, max_recs, rec + i0 * max_recs * 4, cnt + i0); });
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
static int64_t irred_scratch()
{
	const char *e = getenv("RB2_IRRED_SCRATCH");
	const int64_t v = e ? atoll(e) : 0;
	return v > 0 ? std::min(v, IRRED_SCRATCH_BYTES) : IRRED_SCRATCH_BYTES;
}

/* n queries, all device pointers, none that counts longer than lmax symbols: one launch, the stacks sized from the entries a row can hold */
static void launch_irreducible(rb2_hip_t *h, int64_t n, const uint8_t *qry, const int64_t *off, int64_t base, int64_t lmax, int64_t min_ovlp, int64_t max_ext,
                               int64_t max_steps, int64_t max_recs, int64_t *rec, int64_t *cnt)
{
	const int64_t cap = irred_entry_cap(lmax, min_ovlp, max_ext, max_steps), row = irred_row_bytes(cap, max_ext), rows = irred_rows(n, row, irred_scratch());
	h->qscr.ensure((size_t)(rows * row));
	qlaunch(h, k_irreducible<true>, k_irreducible<false>, (uint64_t)rows, qry, off, base, n, min_ovlp, max_ext, max_steps, max_recs, lmax, rows, cap, h->qscr.p, rec, cnt);
}

static void irreducible_check(const char *who, int64_t max_len, int64_t min_ovlp, int64_t max_ext, int64_t max_steps, int64_t max_recs)
{
	if (min_ovlp < 1) { rb2_fatal("[rb2_hip] %s: min_ovlp must be at least 1 (got %lld)\n", who, (long long)min_ovlp); }
	if (max_ext < 1 || max_ext > IRRED_MAX_LEN) { rb2_fatal("[rb2_hip] %s: max_ext must be 1 .. %lld (got %lld)\n", who, (long long)IRRED_MAX_LEN, (long long)max_ext); }
	if (max_steps < 1) { rb2_fatal("[rb2_hip] %s: max_steps must be at least 1 (got %lld)\n", who, (long long)max_steps); }
	if (max_recs < 1) { rb2_fatal("[rb2_hip] %s: max_recs must be at least 1 (got %lld)\n", who, (long long)max_recs); }
	if (max_len < 1 || max_len > IRRED_MAX_LEN) { rb2_fatal("[rb2_hip] %s: max_len must be 1 .. %lld (got %lld)\n", who, (long long)IRRED_MAX_LEN, (long long)max_len); }
}

int64_t rb2_hip_irreducible(rb2_hip_t *h, int64_t n, const uint8_t *qry, const int64_t *off, int64_t min_ovlp, int64_t max_ext, int64_t max_steps, int64_t max_recs,
                            int64_t *rec, int64_t *cnt)
{
	query_begin(h, "irreducible");
	if (n <= 0) return 0;
	irreducible_check("irreducible", 1, min_ovlp, max_ext, max_steps, max_recs);
	check_offsets("irreducible", "query", n, off);
	int64_t lmax = 1;                                              // the longest query that is not malformed by its length alone
	for (int64_t i = 0; i < n; ++i) if (off[i + 1] - off[i] <= IRRED_MAX_LEN) lmax = std::max(lmax, off[i + 1] - off[i]);
	return staged_records(h, n, {qry, off, 0}, 4, max_recs, rec, cnt, [&](int64_t nc, const QStaged &s, int64_t *d_rec, int64_t *d_cnt) {
		launch_irreducible(h, nc, s.bytes, s.v, s.base, lmax, min_ovlp, max_ext, max_steps, max_recs, d_rec, d_cnt); },
		[](int64_t c) { return c >= 0 ? c : c <= -2 ? -2 - c : 0; });     // a query that ran out of steps keeps what it had found
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
