/* rb2_hip.h -- C ABI of the MI355X (gfx950) multi-string BWT insertion engine.
 *
 * This is the drop-in boundary for ropebwt2's hot path.  The host side stays plain C; every
 * symbol below is `extern "C"`, takes plain pointers and sizes, and is what the `mrope` layer
 * (include/mrope.h, our replacement for /root/reference/mrope.h) binds to:
 *
 *   reference interface replaced                         entry point here
 *   ---------------------------------------------------  -----------------------------------------
 *   mr_insert_multi()            mrope.c:258-345         rb2_hip_insert_multi[_dev]()
 *     mr_insert_multi_aux()      mrope.c:184-233           (k_prep / k_merge / k_advance kernels)
 *     rope_insert_run()          rope.c:114-148            (k_merge: rank + positional insert)
 *     rope_rank2a()              rope.c:179-194            (k_prep: interval sizes)
 *     rle_insert_cached/rank2a   rle.c:10-89, 134-191      (k_merge: run-length leaf decode/encode)
 *   rope_t.c[6] marginal counts  rope.h:19, mrope.h:86   rb2_hip_get_counts()
 *   mr_itr_first/next_block      mrope.c:111-130         rb2_hip_rope_bytes() + rb2_hip_download_rope()
 *   mr_restore / rope_restore    mrope.c:145, rope.c:308 rb2_hip_load_ropes()
 *   rld_restore                  rld0.c:246-300          rb2_hip_load_fmd[_file]()
 *   rld_enc .. rld_dump          rld0.c:107-244          rb2_hip_save_fmd[_file]()
 *
 * Run-length byte streams crossing this boundary use ropebwt2's "43+3" codec (rle.h:39-75), so
 * the host can splice them straight into rope leaves.  The device itself only ever emits the
 * 1-byte form (run length < 16), which is a valid subset of that codec.
 *
 * Limits of this build (checked; a violation prints a message and abort()s):
 *   - fewer than 2^32 - 1024 strings per batch (string ids are 32 bit on the device; ropebwt2's default -m10g holds at most
 *     ~10^10 one-symbol strings, so this only excludes batches of degenerate reads);
 *   - positions inside one sub-rope below 2^48 (the sharded wire format packs l into 48 bits, rb2_device.h ShardRec);
 *   - at most 64 ranks in the sharded protocol (RB2_MULTI_MAX_RANKS; 31 sub-ropes exist; more than 16 ranks carry no additional load on DNA);
 *   - one dense merge launch covers at most 2^32 threads = 2^26 windows of 5376 symbols: about 360 G symbols per GPU and round
 *     (checked per round, with a message); larger indexes are what the sharded build is for;
 *   - in-place (sparse) rounds are used for batches of fewer than 2^27 strings (one wave per four touched leaves in one launch);
 *     larger batches simply stay on the dense path -- a performance boundary, not an error;
 *   - leaf slots of one pool are addressed with 32 bits in the sparse layout (the work orders, the split list): 2^32 slots = 4.3 T symbols;
 *   - symbols must be nt6 codes 0..5, the buffer must end with a sentinel (mrope.c:268);
 *   - rb2_hip_load_ropes takes at most 2^20 run codes longer than 4096 symbols per rope, rb2_hip_load_fmd at most 2^20 per file
 *     (what counts is the part of one code inside one piece: a run written as several codes counts once per code, a code cut by a
 *     piece border once per part; codes of symbol 0 do not count; the list of parts that get a workgroup of their own has that many slots);
 *   - the index lives in HBM: 2 x 0.38 B per symbol (dense layout) plus ~100 B per string of the batch; running out of device
 *     memory reports the size that was needed.
 *
 * Error convention: like the reference (mrope.c has none), functions do not return error codes
 * for programming errors; any HIP failure or a missing GPU prints a message to stderr and
 * abort()s -- there is no CPU fallback behind this ABI.
 */
#ifndef RB2_HIP_H_
#define RB2_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rb2_hip_s rb2_hip_t;

/* sorting orders, same values as MR_SO_IO / MR_SO_RLO / MR_SO_RCLO (mrope.h:6-8) */
#define RB2_SO_IO   0
#define RB2_SO_RLO  1
#define RB2_SO_RCLO 2

/* Fatal errors (a HIP call that fails, a missing GPU, a malformed batch, out of device memory): a message on stderr, then abort() --
 * the reference's own convention on this path (asserts and unchecked mallocs).  A host program that wants a say
 * installs a handler: it is called with the message before abort() and may log, release what it holds, or leave through longjmp /
 * exit (the handle that failed must not be used again; others may).
 * With N GPUs behind one handle (rb2_hip_multi_*) a failure may be detected on the host thread of the rank it happens on: that
 * thread records the message and ends, the threads of the other ranks leave at their next round barrier, and the handler is called
 * -- once, with the first message -- on the thread that called the API, after all rank threads are joined: the same rules as above. */
typedef void (*rb2_hip_fatal_cb)(void *user, const char *message);
void rb2_hip_set_fatal_handler(rb2_hip_fatal_cb cb, void *user);

/* number of visible HIP devices (0 when there is no GPU; never aborts) */
int rb2_hip_device_count(void);

/* create an empty six-rope BWT on `device` (mr_init, mrope.c:14-25).  abort()s without a GPU. */
rb2_hip_t *rb2_hip_create(int device, int sorting_order);
void rb2_hip_destroy(rb2_hip_t *h);
int  rb2_hip_sorting_order(const rb2_hip_t *h);
/* empty the index again (what mr_destroy + mr_init would do) but keep every buffer the handle has grown */
void rb2_hip_reset(rb2_hip_t *h);

/* mr_insert_multi (mrope.c:258): insert all strings of `s` (concatenated, each REVERSED and
 * 0-terminated, nt6 codes 0..5, s[len-1]==0).  `s` is a host buffer, borrowed for the call. */
void rb2_hip_insert_multi(rb2_hip_t *h, int64_t len, const uint8_t *s);

/* rb2_hip_insert_multi may return as soon as the batch text is on the device and its rounds are queued (default; RB2_HIP_LAZY_INSERT=0
 * or rb2_hip_set_lazy(h, 0): only when the device is done): `s` is the caller's again, and what it does next -- parse the next batch,
 * upload it (the text goes to a second device buffer on a copy stream) -- runs beside the kernels.  Every other entry point waits for
 * the queued rounds before it looks at the index; rb2_hip_wait does only that.  rb2_hip_last_batch_counts: what that batch adds to
 * the count matrix (layout of rb2_hip_get_counts), computed from its text alone and valid at once -- how mr_insert_multi keeps
 * mr_get_c() truthful (mrope.c:332-340) without waiting; returns 0 when the last insert was not a host-buffer one. */
void rb2_hip_set_lazy(rb2_hip_t *h, int on);
void rb2_hip_wait(rb2_hip_t *h);
int  rb2_hip_last_batch_counts(rb2_hip_t *h, int64_t d[36]);

/* optional: bytes [0, n_final) of the buffer a LATER rb2_hip_insert_multi(h, len >= n_final, s) will pass are final -- start
 * uploading them now (copy stream, second text buffer), concurrently with an insert running on another thread.  capacity = the
 * largest len that call may have.  `s` must stay where it is until that call; s == NULL cancels (waits for copies in flight:
 * call it before reallocating or freeing a buffer that was announced).  (The reference reads and inserts in one thread,
 * main.c:238-242; this is what lets the PCIe crossing of batch k+1 hide behind the insertion of batch k.) */
void rb2_hip_prefetch(rb2_hip_t *h, const uint8_t *s, int64_t n_final, int64_t capacity);
/* A caller that hands the same host buffers to rb2_hip_insert_multi again and again (batch after batch, as main.c:238 does with its
 * one read buffer) can page-lock them once: the batch then crosses PCIe by DMA straight from the caller's memory instead of through the
 * runtime's staging copies of pageable memory.  Thin wrappers of hipHostRegister / hipHostUnregister, so that a plain-C host needs no HIP
 * header; 0 on success.  Optional: an unregistered buffer works as before.  (No counterpart in the reference: mrope.c:258 takes a
 * pointer and reads it on the CPU.) */
int rb2_hip_host_register(void *p, int64_t nbytes);
int rb2_hip_host_unregister(void *p);

/* free / total memory of a device in bytes (0, 0 without a usable GPU; never aborts): what `ropebwt2 -m auto` sizes its batches from */
void rb2_hip_mem_info(int device, int64_t *free_bytes, int64_t *total_bytes);

/* same, but `s_dev` already resides in this device's HBM (no PCIe transfer in the call) */
void rb2_hip_insert_multi_dev(rb2_hip_t *h, int64_t len, const uint8_t *s_dev);

/* c[b*6+a] = number of symbol a in rope b == mr->r[b]->c[a] (rope.h:19) */
void rb2_hip_get_counts(rb2_hip_t *h, int64_t c[36]);

/* rope b as a run-length byte stream (43+3 codec, 1-byte runs only).  rb2_hip_rope_bytes gives
 * the exact size; download copies it to host memory `dst` and returns the byte count. */
int64_t rb2_hip_rope_bytes(rb2_hip_t *h, int b);
int64_t rb2_hip_download_rope(rb2_hip_t *h, int b, uint8_t *dst);
/* the same stream handed to a callback in pieces of whole runs (up to 32 MiB per call; the buffer is only valid during
 * the call), without a host copy of the whole rope: what an .fmd / text writer needs (replaces the walk over mr_itr_next_block, mrope.c:114-131) */
typedef void (*rb2_hip_run_cb)(void *user, const uint8_t *runs, int64_t n_bytes);
int64_t rb2_hip_stream_rope(rb2_hip_t *h, int b, rb2_hip_run_cb cb, void *user);

/* replace all six ropes by the symbols described by six 43+3 run-length streams (any run
 * width; rle[b] may be NULL when n_bytes[b]==0).  Used to seed the device from an .fmr file /
 * host ropes (mr_restore, mrope.c:145-160; rope_restore, rope.c:308-318). */
void rb2_hip_load_ropes(rb2_hip_t *h, const uint8_t *const rle[6], const int64_t n_bytes[6]);

/* replace all six ropes by the index an .fmd file holds (fermi's run-length delta BWT, rld0.c:207-244: what `ropebwt2 -d`, this
 * project's CLI and fermi write).  `fmd` is the whole file image in host memory, borrowed for the call.  Like rb2_hip_load_ropes it
 * finishes a lazy insert first and leaves the dense layout; the stream is uploaded once and decoded on the device, one lane per 64-byte
 * block (k_fmd_*, csrc/rb2_fmd_load.h); the rank frames behind the stream are not read.  Returns the number of symbols loaded; a file
 * whose marginal counts are all zero loads as an empty index.  The file does not record a sorting order: the handle keeps the one it was
 * created with, and whether later inserts in that order make sense for this index is the caller's business.
 * Fatal, each with a message of its own: wrong magic; an alphabet other than 6 symbols or blocks other than 8 words; a stream length
 * that is no multiple of 8, or an image shorter than 80 bytes + the stream; an invalid block header; a block whose decoded symbols
 * disagree with the counts in the next header; totals that disagree with the file's marginal counts; a symbol code above 5; ropes
 * that are inconsistent with each other, as for rb2_hip_load_ropes. */
int64_t rb2_hip_load_fmd(rb2_hip_t *h, const void *fmd, int64_t n_bytes);
/* the same for a file that is read into memory first; a file that cannot be opened or read is fatal with its name */
int64_t rb2_hip_load_fmd_file(rb2_hip_t *h, const char *path);

/* ---- the index as an .fmd image (csrc/rb2_fmd_save.h, csrc/rb2_fmd_plan.h) ----
 * The image is fermi's "RLD\3": what `ropebwt2 -d` and rb2_fmd_write produce from the same BWT, byte for byte -- an 80-byte header, the
 * stream of n_bytes (blocks of 8 words: the run-length delta codes of the six ropes one after the other, equal neighbours merged across
 * leaves, pieces and ropes) and n_frames rank frames of 56 bytes.  The SIZE of the image is 80 + n_bytes + 56 n_frames.
 * rb2_hip_save_fmd returns SIZE and writes the image to dst (host memory) only if dst != NULL and cap >= SIZE; otherwise it writes
 * NOTHING, not a byte of dst, and still returns SIZE: a caller sizes with one call and fetches with a second (the handle remembers SIZE
 * until the rows change or a sampled suffix array is built or dropped, so the second call encodes once).  It synchronises before it returns.
 * rb2_hip_save_fmd_file writes the same bytes to path: the stream goes out at its file offset while later parts are still being encoded,
 * the header and the rank frames are written last.  Returns SIZE, or -1 when the file cannot be opened or written -- the caller's error,
 * nothing fatal; what the file holds then is undefined.
 * Both calls leave the index UNCHANGED: the same rows, counts and rope hashes, the sampled suffix array kept; like rb2_hip_stream_rope they
 * finish a lazy insert and may leave a sparse layout for the dense one.  An EMPTY index gives the image the host writer gives for no run at
 * all: the header, an all-zero first block, a closing header of two zero words and one zero frame, 216 bytes.
 * Everything from the bit planes to the finished words happens on the device, in batches of at most 2^24 runs (RB2_FMDS_BATCH lowers
 * that, RB2_FMDS_SEG sets the runs per segment of the block-boundary tables, 96 .. 8192; both are read once per call and exist for tests);
 * the host copies finished bytes out of two pinned buffers.  Device memory for it does not grow with the index: at most 1.3 GB.
 * Runs below 2^51 symbols, as for the host writer and the loader.  One case is outside the byte-for-byte promise: a run of 2^50 symbols or
 * more (a 64-bit code) that arrives right behind a code ending on a word boundary makes the host writer, like rld0.c:145, shift a word by
 * 64, so there is no defined image to equal; the encoder places such a code like any other.  No index a device holds comes near it.  Fatal: one rank of a sharded index; an index of more rows than 2^24
 * rank frames cover (with frames of 2^11 rows, as reads give them, 3.4e10 rows); a block of 2^30 symbols or more right in front of the
 * last block of a chunk of 2^23 words, whose header of seven words leaves that block no payload word (the reference misbehaves there). */
int64_t rb2_hip_save_fmd(rb2_hip_t *h, void *dst, int64_t cap);
int64_t rb2_hip_save_fmd_file(rb2_hip_t *h, const char *path);

/* Take strings out of the index again (no counterpart in the reference, whose ropes only grow).  ids: n string
 * ids in host memory, in any order, duplicates allowed -- a string id is a row of the `$` block, what rb2_hip_extract takes and
 * rb2_hip_locate / rb2_hip_string_ids give; in input order id k is the k-th string inserted.  Afterwards the index is the BWT of the
 * remaining strings, byte for byte what rb2_hip_download_rope gives for an index built from them alone in the same order.  The ids of
 * the survivors close ranks: old id k becomes k minus the number of deleted ids below k.  Returns the rows removed (symbols plus
 * sentinels of the deleted strings), counted on the device.
 * The call finishes a lazy insert first, leaves the dense layout with plain windows, drops the sampled suffix array and returns when
 * the new index is in place; n == 0 returns 0 and changes nothing (not the layout, not the suffix array).  Deleting every string
 * leaves an empty index that takes inserts as after rb2_hip_reset.  Cost: one LF walk per deleted string and one streaming rewrite of
 * the index (k_del_*, csrc/rb2_delete.h); device memory: the second pool side plus 8 bytes of marks per 64 rows and 12 bytes per leaf.
 * Fatal, each with a message of its own and before anything is changed: an id below 0 or not below the number of strings; n < 0; a
 * rank of a sharded index; a walk that does not end within the rows of the index or leaves it (a loaded index that is no BWT of
 * complete strings).
 * rb2_hip_delete_stats: what the last deletion met -- out[0] rows removed, out[1] source groups of 64 rows that held rows, out[2] those
 * of them whose kept rows had to be closed up by the bit compress (the others are copied by a shift), out[3] leaf slots read,
 * out[4] leaf slots written. */
int64_t rb2_hip_delete_strings(rb2_hip_t *h, int64_t n, const int64_t *ids);
void rb2_hip_delete_stats(rb2_hip_t *h, int64_t out[5]);

/* optional capacity hint (like the reference sizing its buffers from -m, main.c:136): make room for batches
 * of up to batch_bytes bytes / batch_strings strings and an index of total_symbols symbols, so that
 * rb2_hip_insert_multi* never has to grow (reallocate + copy) a buffer.  Any argument may be 0. */
void rb2_hip_reserve(rb2_hip_t *h, int64_t batch_bytes, int64_t batch_strings, int64_t total_symbols);

/* rank of all six symbols in [0,x) of rope b, computed on the device (rope_rank1a, rope.h:45) */
void rb2_hip_rank1a(rb2_hip_t *h, int b, int64_t x, int64_t cx[6]);
/* the same for n positions at once: out[i*6 + a] = number of a's in [0, x[i]) of rope b.  One wave per query (a coalesced
 * 512-byte leaf load, bit-plane popcounts per lane, DPP reduction): the query-side counterpart of rope_rank1a for workloads
 * that ask millions of ranks (x, out: host memory). */
void rb2_hip_rank_batch(rb2_hip_t *h, int b, int64_t n, const int64_t *x, int64_t *out);

/* ---- FM-index queries on the device index ---------------------------------------------------
 * The BWT this engine builds is an FM-index of the strings as read (they are inserted reversed, mr_insert_multi).  Coordinates:
 *   rows     global row numbers of the concatenated BWT, rope 0 ($) through rope 5 (N): what the six rb2_hip_download_rope streams
 *            give one after the other, what an .fmd of the index holds.  Rope b is its pieces (b,$), (b,A) .. (b,N) in that order.
 *   C[a]     rows in front of rope a = sum over b < a of row b of rb2_hip_get_counts (e->cnt[a] of rld0 after rld_enc_finish).
 *   occ(a,x) number of a's in global rows [0, x): the counts of the pieces in front of x plus a rank inside the piece that holds x.
 *   pattern  nt6 codes in text order: 1..5 anywhere, 0 ($) only as the last symbol, where it anchors the pattern at a string end.
 *            Backward search consumes a pattern from its last symbol.
 * Every query waits for a lazy insert first (as every entry point does), reads the index and nothing else, and is fatal on one rank of a
 * sharded index (rb2_hip_multi_*), like rb2_hip_rank_batch.  The host variants stage through device buffers in chunks of at most 2^24
 * queries (RB2_QUERY_CHUNK in the environment lowers it: tests).  Kernels: k_bsearch, k_extend, k_extract (csrc/rb2_query.h). */
/* n patterns concatenated in pat[off[i] .. off[i+1]) (off: n + 1 non-decreasing values); out[3*i ..] = lo, hi, m: m is the length of the
 * longest suffix of pattern i that occurs and [lo, hi) its interval, so count = hi - lo when m == the pattern's length, else 0.  The empty
 * pattern gives (0, N, 0), N = rows; a malformed pattern (a code above 5, a `$` before its end) gives (-1, -1, -1) and is not an error. */
void rb2_hip_backward_search(rb2_hip_t *h, int64_t n, const uint8_t *pat, const int64_t *off, int64_t *out);
/* the same with pat, off and out in this device's memory, asynchronous on the handle's stream */
void rb2_hip_backward_search_dev(rb2_hip_t *h, int64_t n, const uint8_t *pat, const int64_t *off, int64_t *out);
/* rld_extend (rld0.c:474-490) on n bi-intervals ik[3*i ..] = x[0], x[1], x[2] (size): ok[18*i + 3*a + j] = x[j] of the extension by
 * a, x[is_back] in the complement order $ T G C A N.  Meaningful when the index holds both strands of every string (as fermi requires):
 * the caller's responsibility. */
void rb2_hip_extend(rb2_hip_t *h, int64_t n, const int64_t *ik, int is_back, int64_t *ok);
/* inverse BWT from rows of the $ block [0, C[1]): the string of row rows[i] in text order into out[i*max_len ..), len[i] its length,
 * -1 when it is longer than max_len, -2 for a row outside the $ block.  In input order (RB2_SO_IO) row k is the k-th string inserted.
 * Returns the number of rows whose string fitted. */
int64_t rb2_hip_extract(rb2_hip_t *h, int64_t n, const int64_t *rows, int64_t max_len, uint8_t *out, int64_t *len);
/* super-maximal exact matches (SMEMs) of n queries against an index that holds both strands of every string (the caller's responsibility,
 * as for rb2_hip_extend; on any other index the results are unspecified, but the call returns and stays in bounds).  Queries are nt6 codes
 * in text order, concatenated in qry[off[i] .. off[i+1]): 1..4 can be matched, 5 (N) is legal but belongs to no match, 0 or a code above 5
 * makes the query malformed.  With occ(s,e) = occurrences of q[s:e) and e(s) = the largest e with occ(s,e) >= min_occ (s if none),
 * [s, e(s)) is an SMEM when e(s) > s, s == 0 or e(s-1) < e(s), and e(s) - s >= min_len: a match with at least min_occ occurrences that
 * cannot be extended on either side and lies inside no other such match.  They are reported in increasing s (their ends increase too).
 * mem[(i*max_mems + k)*5 ..] = start, end, x0, x1, size of the k-th SMEM of query i, (x0, x1, size) its bi-interval in the coordinates of
 * rb2_hip_extend: x0 = lo of backward_search(q[start:end)), x1 = lo of its reverse complement, size = hi - lo.  cnt[i] = SMEMs found,
 * which may exceed max_mems (the surplus is counted, not stored), or -1 for a malformed query.  Only the first min(cnt[i], max_mems)
 * records of a query are meaningful: the host variant returns the others as zeros, the device variant leaves them untouched.
 * min_len, min_occ and max_mems below 1 are fatal.  Returns the number of records stored (sum of min(cnt[i], max_mems), malformed queries
 * counting 0).  The host variant lowers its chunk further so that the records staged for one chunk (chunk * max_mems * 40 bytes) stay
 * under 256 MiB, one query at the least: it never allocates n * max_mems records on the device at once.  Kernel: k_smem. */
int64_t rb2_hip_smem(rb2_hip_t *h, int64_t n, const uint8_t *qry, const int64_t *off, int64_t min_len, int64_t min_occ, int64_t max_mems,
                     int64_t *mem, int64_t *cnt);
/* the same with qry, off, mem and cnt in this device's memory, asynchronous on the handle's stream (no return value: read cnt) */
void rb2_hip_smem_dev(rb2_hip_t *h, int64_t n, const uint8_t *qry, const int64_t *off, int64_t min_len, int64_t min_occ, int64_t max_mems,
                      int64_t *mem, int64_t *cnt);

/* ---- sampled suffix array: from rows back to places in the strings ----
 * String id k = the row of the $ block rb2_hip_extract takes (in input order the k-th string inserted); n = C[1] strings.  The walk of k
 * starts at row k and takes LF steps until the BWT symbol is `$`; the row after j steps is the suffix of string k that starts j symbols
 * before its end.  Every row lies on exactly one walk, and SA(row) = (k, len[k] - j): the string and the 0-based position in text order
 * where the row's suffix starts; for the rows of the $ block that is (k, len[k]), the place of the sentinel.
 * rb2_hip_ssa_build walks every string once (k_ssa_build) and keeps (k, j) of every row x with x % 2^log2_step == 0, the length of every
 * string, and the string behind every whole-string row: 16 bytes per sample and 16 per string of device memory.  It returns the samples
 * stored, ceil(N / 2^log2_step); an empty index gives 0.  log2_step outside 0 .. 30 is fatal.  The array describes the rows as they are
 * now: an insert, rb2_hip_load_ropes, rb2_hip_load_fmd*, rb2_hip_delete_strings and rb2_hip_reset drop it (rb2_hip_ssa_drop does so on request and frees its
 * memory, rb2_hip_destroy too); a change between the dense and the sparse layout does not.  Building again replaces it.
 * rb2_hip_ssa_info: out[0] 1 when an array is valid, out[1] its log2_step, out[2] its samples, out[3] the bytes of device memory held. */
int64_t rb2_hip_ssa_build(rb2_hip_t *h, int log2_step);
void    rb2_hip_ssa_drop(rb2_hip_t *h);
void    rb2_hip_ssa_info(rb2_hip_t *h, int64_t out[4]);
/* n intervals of rows iv[2*i], iv[2*i+1] = lo, hi (what backward_search, extend and smem return): hit[(i*max_hits + k)*2 ..] = string id,
 * position of row lo + k for k < min(hi - lo, max_hits), in row order; cnt[i] = hi - lo, which may exceed max_hits (the surplus is counted,
 * not stored), or -1 for lo < 0, hi > N or lo > hi (not an error).  Each row walks LF to the nearest sample or string end (k_locate): at
 * most the length of its string, about 2^log2_step steps in a BWT of many strings.  Only the first min(cnt[i], max_hits) records of an
 * interval are meaningful: the host variant returns the others as zeros, the device variant leaves them untouched.  Without a valid array
 * the call is fatal (the message names rb2_hip_ssa_build); max_hits < 1 is fatal.  Returns the number of records stored.  The host variant
 * stages chunks whose records (chunk * max_hits * 16 bytes) stay under 256 MiB, one interval at the least. */
int64_t rb2_hip_locate(rb2_hip_t *h, int64_t n, const int64_t *iv, int64_t max_hits, int64_t *hit, int64_t *cnt);
/* the same with iv, hit and cnt in this device's memory, asynchronous on the handle's stream (no return value: read cnt) */
void    rb2_hip_locate_dev(rb2_hip_t *h, int64_t n, const int64_t *iv, int64_t max_hits, int64_t *hit, int64_t *cnt);

/* ---- suffix-prefix overlaps: which strings of the index begin with a suffix of a query ----
 * A row of the interval [lo, hi) of a non-empty pattern P whose BWT symbol is `$` is the row of a whole string that starts with P: the
 * index holds occ($,hi) - occ($,lo) strings with the prefix P, and the `$` ranks q in [occ($,lo), occ($,hi)) name them.
 * rb2_hip_overlap: n queries as for rb2_hip_smem (nt6 codes in text order, concatenated in qry[off[i] .. off[i+1]); 1..4 match; 5 (N) is
 * legal but belongs to no overlap: the search of a query stops at the first N met from the query's end; 0 or a code above 5 makes the query
 * malformed).  For every length l, min_ovlp <= l <= len, whose suffix q[len-l ..) occurs and is the prefix of at least one string there is
 * one record rec[(i*max_recs + k)*3 ..] = l, zlo, zhi, in increasing l: [zlo, zhi) is the range of `$` ranks of those strings (zhi - zlo
 * of them; rb2_hip_string_ids names them).  l == len is reported too: the query itself when it is in the index, its copies, and the strings
 * it is a proper prefix of.  cnt[i] = records found, which may exceed max_recs (the surplus is counted, not stored; len - min_ovlp + 1
 * always suffices), 0 for the empty query, -1 for a malformed one.  Only the first min(cnt[i], max_recs) records of a query are meaningful:
 * the host variant returns the others as zeros, the device variant leaves them untouched.  min_ovlp and max_recs below 1 are fatal.
 * Returns the number of records stored.  No suffix array is needed.  The index may hold one strand or both: the reverse-complement overlaps
 * of a query are the overlaps of its reverse complement on an index of both strands.  One backward search per query whose every step reads
 * the `$` counts along with the step's own (k_overlap): at most len rank pairs.  The host variant stages chunks whose records (chunk *
 * max_recs * 24 bytes) stay under 256 MiB, one query at the least. */
int64_t rb2_hip_overlap(rb2_hip_t *h, int64_t n, const uint8_t *qry, const int64_t *off, int64_t min_ovlp, int64_t max_recs, int64_t *rec, int64_t *cnt);
/* the same with qry, off, rec and cnt in this device's memory, asynchronous on the handle's stream (no return value: read cnt) */
void    rb2_hip_overlap_dev(rb2_hip_t *h, int64_t n, const uint8_t *qry, const int64_t *off, int64_t min_ovlp, int64_t max_recs, int64_t *rec, int64_t *cnt);
/* n ranges of `$` ranks zv[2*i], zv[2*i+1] = zlo, zhi (what rb2_hip_overlap returns): ids[i*max_hits + k] = the string behind the
 * (zlo + k)-th `$` of the BWT for k < min(zhi - zlo, max_hits), ids as in rb2_hip_extract and rb2_hip_locate; cnt[i] = zhi - zlo, which may
 * exceed max_hits (the surplus is counted, not stored), or -1 for zlo < 0, zhi > the number of strings or zlo > zhi (not an error).  Only
 * the first min(cnt[i], max_hits) ids of a range are meaningful: the host variant returns the others as zeros, the device variant leaves
 * them untouched.  A gather from the suffix array's table of whole-string rows (k_string_ids), so it needs a valid array of any log2_step:
 * without one the call is fatal (the message names rb2_hip_ssa_build); max_hits < 1 is fatal.  Returns the number of ids stored.  The host
 * variant stages chunks whose ids (chunk * max_hits * 8 bytes) stay under 256 MiB, one range at the least. */
int64_t rb2_hip_string_ids(rb2_hip_t *h, int64_t n, const int64_t *zv, int64_t max_hits, int64_t *ids, int64_t *cnt);
/* the same with zv, ids and cnt in this device's memory, asynchronous on the handle's stream (no return value: read cnt) */
void    rb2_hip_string_ids_dev(rb2_hip_t *h, int64_t n, const int64_t *zv, int64_t max_hits, int64_t *ids, int64_t *cnt);

/* ---- k-mer enumeration: which k-mers the indexed strings contain, and how often ----
 * A k-mer is k consecutive symbols of one indexed string, all of them A C G T (nt6 codes 1 .. 4): a window that holds an N, or that would
 * run over the end of its string, is none.  Its count is hi - lo of rb2_hip_backward_search on it, so an index of both strands counts both
 * strands.  rb2_hip_kmers reports every distinct k-mer with at least min_occ occurrences (what `fermi2 count` lists; the k-mer spectrum).
 * rec[3*j ..] = code, lo, hi for j < min(return value, max_recs): code packs the k-mer two bits per symbol, A = 0 C = 1 G = 2 T = 3, the
 * symbol at text position p at bits 2 * (k - 1 - p), so that the numeric order of the codes (taken as unsigned) is the lexicographic order
 * of the k-mers, which is also the order of their lo; [lo, hi) is the k-mer's interval in the global rows of the other queries and can be
 * handed to rb2_hip_locate as it is.  The order of the records is unspecified.  Returns the number of k-mers found, which may exceed
 * max_recs (the surplus is counted, not stored): exactly max_recs records are stored then, every one a true record, none twice; which ones
 * is unspecified, and rec beyond the records stored is left untouched.
 * hist[c], c < hist_len - 1 = the reported k-mers with exactly c occurrences, hist[hist_len - 1] = those with hist_len - 1 or more:
 * complete whatever max_recs is (max_recs = 0 gives the spectrum alone); the bins below min_occ are zero.
 * canonical != 0: a k-mer is reported only if its code <= the code of its reverse complement (a palindrome once); the count stays that of
 * the k-mer itself.  Meaningful on an index of both strands, where the two counts agree: the caller's responsibility, as for rb2_hip_extend.
 * info (may be NULL): [0] expand launches, [1] the largest number of items in a frontier segment, [2] the largest number of segments alive
 * at once, [3] the k-mers that met min_occ before the canonical filter.
 * rec may be NULL when max_recs == 0, hist when hist_len == 0.  Fatal: k outside 1 .. 32, min_occ < 1, max_recs < 0 or hist_len < 0, a NULL
 * pointer with a size that is not 0.  An empty index gives 0 and a histogram of zeros.  Like every query the call reads the index and
 * nothing else: a sampled suffix array stays valid across it.
 * The enumeration is level-wise (k_kmer_expand: the two ranks of an l-mer's interval give the intervals of its four left extensions; an
 * extension below min_occ is dropped for good) and walks the levels depth-first over segments of at most F items, so it holds k * F * 24
 * bytes of device memory at the most whatever the index (F = RB2_KMER_FRONTIER in the environment, at least 4, 2^22 by default); the
 * records are staged on the device and copied out in pieces of at most 256 MiB.  There is no _dev variant: the host sizes every launch
 * from the count the one before it wrote, so the call cannot be asynchronous. */
int64_t rb2_hip_kmers(rb2_hip_t *h, int k, int64_t min_occ, int canonical, int64_t max_recs, int64_t *rec, int64_t hist_len, int64_t *hist, int64_t info[4]);

/* ---- approximate search: the matches of a query within a bounded number of substitutions ----
 * rb2_hip_approx: n queries as for rb2_hip_smem (nt6 codes in text order, concatenated in qry[off[i] .. off[i+1]); 1..4 can match; 5 (N) is
 * legal and matches nothing: an N position is always a substitution, by any of A C G T; 0, a code above 5 or a length above 8192 makes the
 * query malformed).  A match of a query of L symbols is a word S of L symbols out of A C G T with at most max_mm positions where
 * S[p] != q[p] and at least min_occ occurrences, occurrences = hi - lo of rb2_hip_backward_search on S.  Every match is reported exactly
 * once, as one record rec[(i*max_recs + k)*4 ..] = lo, hi, n_mm, subs: [lo, hi) is the interval of S in global rows and can be handed to
 * rb2_hip_locate as it is; n_mm is the number of substitutions; subs packs them 16 bits each as pos << 3 | sym -- the text position and the
 * nt6 code S has there -- in decreasing pos (the order a backward search meets them), the first in bits 0 .. 15.  Unused fields are 0, a
 * used one never is (sym >= 1).  The order of a query's records is unspecified.
 * cnt[i] >= 0: the matches found, which may exceed max_recs: exactly max_recs records are stored then, every one a true record, none
 * twice; which ones is unspecified.  0 for the empty query, -1 for a malformed one.  cnt[i] <= -2: the query used up max_steps before its
 * search ended -- a step is one pair of ranks --; -2 - cnt[i] matches had been found by then and min(-2 - cnt[i], max_recs) of them are
 * stored, every one a true record, none twice.  max_steps is what keeps one query (a homopolymer against a repetitive index at max_mm = 4
 * has millions of nodes) from occupying the device: a call ends after n * max_steps rank pairs whatever the index holds.
 * Only the records stored are meaningful: the host variant returns the others as zeros, the device variant leaves them untouched.
 * Returns the number of records stored.  Fatal: max_mm outside 0 .. 4; min_occ, max_steps or max_recs below 1 (n <= 0 returns first).
 * The index may hold one strand or both: the reverse-complement hits of a query are the hits of its reverse complement on an index of both
 * strands.  No suffix array is needed, and one that is there stays valid: like every query the call reads the index and nothing else.
 * Depth-first backtracking over the positions L-1 .. 0 (k_approx), one query per 16 lanes: the two ranks of a node's interval give its four
 * children; a child is dropped when it has fewer than min_occ rows or when the substitutions so far, its own and a lower bound for the
 * positions in front of it exceed max_mm.  The bound comes from one plain backward search over the query (at most L steps, counted like
 * the others): the query is cut into disjoint pieces that each occur fewer than min_occ times, and every match must change every piece.
 * The stacks live in device memory, 66 bytes per symbol of the longest query and row of the launch, 256 MiB at the most
 * (RB2_APPROX_SCRATCH in the environment lowers that; rows take further queries a launch apart); when the queries are many and the
 * longest is long, those of up to 248 symbols run in a launch of their own on many rows.  The host variant stages chunks whose records
 * (chunk * max_recs * 32 bytes) stay under 256 MiB, one query at the least. */
int64_t rb2_hip_approx(rb2_hip_t *h, int64_t n, const uint8_t *qry, const int64_t *off, int max_mm, int64_t min_occ, int64_t max_steps, int64_t max_recs, int64_t *rec, int64_t *cnt);
/* the same with qry, off, rec and cnt in this device's memory, asynchronous on the handle's stream (no return value: read cnt).  The host
 * does not see the lengths, so the stacks are sized for 8192 symbols: always 256 MiB once there are more than some 500 queries */
void    rb2_hip_approx_dev(rb2_hip_t *h, int64_t n, const uint8_t *qry, const int64_t *off, int max_mm, int64_t min_occ, int64_t max_steps, int64_t max_recs, int64_t *rec, int64_t *cnt);

/* ---- approximate search with insertions and deletions: the matches of a query within a bounded edit distance ----
 * rb2_hip_approx_ed: n queries as for rb2_hip_approx (nt6 codes 1..5 in text order, concatenated in qry[off[i] .. off[i+1]); an N (5) is legal
 * and equals nothing; 0, a code above 5 or a length above 8192 makes the query malformed).
 * Distance.  sub(a, c) = 0 if a == c and c is one of A C G T, else 1.  lev(X, Y) is the unit-cost Levenshtein distance with sub as the cost of
 * a column; deleting an N of the query costs 1 like any other symbol.  For a query q of L symbols and a word S over A C G T:
 *   L >= 2 and |S| >= 2:   ed(S, q) = sub(S[0], q[0]) + lev(S[1:-1], q[1:-1]) + sub(S[-1], q[-1])
 *   L == 1 and |S| == 1:   ed(S, q) = sub(S[0], q[0])
 *   otherwise              ed(S, q) is infinite
 * so the first and the last symbols of a match are aligned to the first and the last symbols of the query: without that every hit S would
 * drag along S[1:], S[:-1], xS, Sx, ... at one more edit each.
 * A match of q is a word S with ed(S, q) <= max_ed and at least min_occ occurrences, occurrences = hi - lo of rb2_hip_backward_search on S.
 * Every match is reported exactly once, as one record rec[(i*max_recs + k)*4 ..] = lo, hi, ed, len: [lo, hi) is the interval of S in global
 * rows and can be handed to rb2_hip_locate as it is; ed = ed(S, q), the minimum and not the cost of some particular alignment; len = |S|,
 * L - max_ed <= len <= L + max_ed.  The alignment itself is not reported: locate and len give the text.  The order of a query's records is
 * unspecified.
 * cnt[i] >= 0: the matches found, which may exceed max_recs: exactly max_recs records are stored then, every one a true record, none
 * twice; which ones is unspecified.  0 for the empty query, -1 for a malformed one.  cnt <= -2: the query used up max_steps before its
 * search ended -- a step is one pair of ranks, and those of the bound count --; -2 - cnt[i] matches had been found by then and
 * min(-2 - cnt[i], max_recs) of them are stored, every one a true record, none twice: the convention of rb2_hip_approx.  A call ends after
 * n * max_steps rank pairs whatever the index holds.
 * Only the records stored are meaningful: the host variant returns the others as zeros, the device variant leaves them untouched.
 * Returns the number of records stored.  Fatal: max_ed outside 0 .. 4; min_occ, max_steps or max_recs below 1 (n <= 0 returns first); one
 * rank of a sharded index.
 * Two identities: at max_ed = 0 the records are (lo, hi, 0, L) of the backward search; and every match of rb2_hip_approx at max_mm = k is
 * a match here at max_ed = k, with ed <= n_mm and len = L (with anchored ends the Hamming alignment is one of the alignments).
 * Depth-first search over the trie of words, built from the last symbol (k_approx_ed), one query per 16 lanes: below the last symbol z a
 * node W'z carries the column D[j] = lev(W', q[1 + j .. L - 1)), of which only the nine cells around the diagonal can hold max_ed or less:
 * nine 4-bit fields of one word.  The two ranks of a node's interval give its four children a; a child with min_occ rows is a match when
 * sub(z, q[L-1]) + D[0] + sub(a, q[0]) <= max_ed, and is followed when some cell of its own column, with a lower bound for the symbols in
 * front of the cell, stays within max_ed.  The bound is that of rb2_hip_approx: one plain backward search cuts the query into disjoint
 * pieces that each occur fewer than min_occ times, and an alignment that leaves a piece untouched would make S contain it.
 * The stacks live in device memory, 74 bytes per symbol of the longest query (plus max_ed) and row of the launch, 256 MiB at the most
 * (RB2_APPROX_SCRATCH in the environment lowers that; rows take further queries a launch apart); when the queries are many and the
 * longest is long, the short ones run in a launch of their own on many rows.  The host variant stages chunks whose records (chunk *
 * max_recs * 32 bytes) stay under 256 MiB, one query at the least (RB2_QUERY_CHUNK lowers the chunk). */
int64_t rb2_hip_approx_ed(rb2_hip_t *h, int64_t n, const uint8_t *qry, const int64_t *off, int max_ed, int64_t min_occ, int64_t max_steps, int64_t max_recs, int64_t *rec, int64_t *cnt);
/* the same with qry, off, rec and cnt in this device's memory, asynchronous on the handle's stream (no return value: read cnt).  The host
 * does not see the lengths, so the stacks are sized for 8192 symbols */
void    rb2_hip_approx_ed_dev(rb2_hip_t *h, int64_t n, const uint8_t *qry, const int64_t *off, int max_ed, int64_t min_occ, int64_t max_steps, int64_t max_recs, int64_t *rec, int64_t *cnt);

/* ---- duplicate and contained strings: which strings an overlap graph, a unitig builder or a dedup step drops first ----
 * For string k (ids as in rb2_hip_extract: rows of the `$` block) with text S, |S| >= 1, symbols compared as codes (an N equals only an N):
 *   occ      occurrences of S as a substring of all indexed strings, itself included: hi - lo of rb2_hip_backward_search on S
 *   n_equal  strings whose text is exactly S, itself included
 *   rank     the position of k among those n_equal strings in row order; exactly one string of every class has rank 0 (in input order
 *            the one with the lowest id)
 *   flag     bit 0 (1): rank > 0 -- a copy of a string that stands before it; bit 1 (2): occ > n_equal -- S lies inside a longer string,
 *            or twice inside one.  4: the empty string (every other field 0).  -1: an id outside [0, C[1]).  -2: the walk left the index
 *            or did not end within N steps (a loaded index that is no BWT of complete strings).  Neither -1 nor -2 is an error, and both
 *            leave the other fields 0.
 *   walked   the LF steps taken: |S| whenever flag is 1, 2 or 3, possibly fewer for flag 0
 * rb2_hip_contained: rec[5*i ..] = flag, occ, n_equal, rank, walked of string ids[i]; ids == NULL means the ids 0 .. n-1 (n = C[1] for the
 * whole index; a surplus gives flag -1).  Returns the number of records with a flag in 1 .. 4: the strings rb2_hip_delete_strings would
 * take out to leave every text once and inside no other.  n < 0 is fatal, n == 0 returns 0.
 * One fused walk per string (k_contain), one string per 16 lanes: the walk of k starts at row k, [lo, hi) = [0, N), ahi = C[1]; a step
 * reads the symbol c of the row, stops at `$`, and otherwise moves row, lo, hi and ahi each to C[c] + occ(c, .).  After j steps [lo, hi) is
 * the interval of the last j symbols of S and [lo, ahi) that of those symbols followed by `$` (`$` sorts first), lo <= row < ahi <= hi.  At
 * the `$`: occ = hi - lo, n_equal = occ($,ahi) - occ($,lo), rank = occ($,row) - occ($,lo).  As soon as hi - lo == 1 after a step the
 * suffix read so far occurs once, so S does: the walk stops with flag 0, occ = n_equal = 1, rank 0 -- after about log4(N) symbols for a
 * string that is no copy and lies in no other.  RB2_CONTAIN_EARLY=0 in the environment, read on every call, turns that exit off (tests).
 * Like every query the call reads the index and nothing else (the layout and a sampled suffix array stay as they are), waits for a lazy
 * insert and is fatal on one rank of a sharded index; the host variant stages chunks of at most 2^24 ids (RB2_QUERY_CHUNK lowers it). */
int64_t rb2_hip_contained(rb2_hip_t *h, int64_t n, const int64_t *ids, int64_t *rec);
/* the same with ids (or NULL) and rec in this device's memory, asynchronous on the handle's stream (no return value: read the flags) */
void    rb2_hip_contained_dev(rb2_hip_t *h, int64_t n, const int64_t *ids, int64_t *rec);

/* ---- irreducible overlaps: the edges of a string graph, transitive reduction included ----
 * n queries as for rb2_hip_approx (nt6 codes 1..5 in text order, concatenated in qry[off[i] .. off[i+1]); 0, a code above 5 or a length above
 * 8192 makes the query malformed).  A candidate of a query q of L symbols is (T, l, X): T a string of the index, min_ovlp <= l < L,
 * T[:l] == q[L-l:] with no N in it (as in rb2_hip_overlap the search stops at the first N from the end), X = T[l:] with 1 <= |X| <= max_ext
 * and only A C G T in it.  l == L is no candidate, nor is a string that is a proper suffix of q (|X| = 0).  A candidate (T, l, X) is
 * reducible when another candidate (U, l', X') has X' a proper prefix of X, or X' == X and l' > l: q reaches T through U.  Every other
 * candidate is irreducible, and there is one record per distinct (l, X) among those: rec[(i*max_recs + k)*4 ..] = l, ext, zlo, zhi with
 * ext = |X|.  [zlo, zhi) is a range of `$` ranks for rb2_hip_string_ids, and THE STRINGS IT NAMES ARE THE REVERSE COMPLEMENTS revcomp(T)
 * OF THE NEIGHBOURS, NOT THE NEIGHBOURS T THEMSELVES: the extension runs over the twin interval, the interval of the reverse complement,
 * and that is what it yields.  On an index of both strands there are exactly zhi - zlo strings T (where a read and its reverse complement
 * are the strings 2i and 2i + 1, T = id ^ 1).  The order of a query's records is unspecified.
 * cnt[i] >= 0: the records found, which may exceed max_recs: exactly max_recs are stored then, every one a true record, none twice.  0 for
 * the empty query, -1 for a malformed one.  cnt[i] <= -2: the query used up max_steps -- a step is one pair of ranks -- with -2 - cnt[i]
 * records found by then and min(-2 - cnt[i], max_recs) of them stored, every one true, none twice: the convention of rb2_hip_approx.
 * Only the records stored are meaningful: the host variant returns the others as zeros, the device variant leaves them untouched.
 * Returns the number of records stored.  Fatal: min_ovlp, max_steps or max_recs below 1; max_ext outside 1 .. 8192 (n <= 0 returns first).
 * The arithmetic (k_irreducible, one query per 16 lanes; it is the same on any BWT, and on an index of one strand the records are
 * whatever it gives: the call returns and stays in bounds):
 *   1. the backward search of rb2_hip_overlap, carrying the bi-interval: (x0, x1, size) = (C[c], C[comp c], C[c+1] - C[c]) for the last
 *      symbol c.  The turn of the last m symbols takes the ranks at x0 and x0 + size; with nd the `$`s between them, min_ovlp <= m < L and
 *      nd > 0 add the entry (m, lo = x1, hi = x1 + nd), the interval of revcomp(q[L-m:]) followed by `$`; then the step by q[L-1-m] moves
 *      x0 and size as a backward search does and x1 as rb2_hip_extend does, in the complement order $ T G C A N.  The search ends behind
 *      the turn of m == L, at an N, or when the interval empties: at most L steps.
 *   2. depth first over the extensions: a node is a depth d and a list of entries (l, lo, hi); the root is the list of 1.  Visiting a
 *      node takes the ranks cl, ch at lo, hi of every entry, one step each.  If d >= 1 and some entry has ch[$] > cl[$], the record
 *      (l, d, cl[$], ch[$]) of the one with the largest l among those is reported and the node is closed.  Otherwise, if d < max_ext, its
 *      child for a = A, C, G, T in that order is the list of the non-empty (l, C[a] + cl[a], C[a] + ch[a]): the extension by comp(a).
 *   3. before every step, a query that has taken max_steps ends over budget.
 * The stacks live in device memory: 66 bytes per entry, min((Lmax - min_ovlp) * (max_ext + 1), max_steps) entries per row of the launch,
 * 256 MiB at the most for all rows (RB2_IRRED_SCRATCH in the environment, read on every call, lowers that; a single row may be larger
 * alone; rows take further queries a launch apart, and the results depend on none of this).  Lmax is the longest query of the call.  The
 * host variant stages chunks whose records (chunk * max_recs * 32 bytes) stay under 256 MiB, one query at the least.
 * Like every query the call waits for a lazy insert, reads the index and nothing else (a sampled suffix array stays valid, and none is
 * needed), and is fatal on one rank of a sharded index. */
int64_t rb2_hip_irreducible(rb2_hip_t *h, int64_t n, const uint8_t *qry, const int64_t *off, int64_t min_ovlp, int64_t max_ext, int64_t max_steps, int64_t max_recs,
                            int64_t *rec, int64_t *cnt);
/* the same with qry, off, rec and cnt in this device's memory, asynchronous on the handle's stream (no return value: read cnt).  The host
 * does not see the lengths: the stacks are sized for max_len symbols (1 .. 8192, anything else is fatal), and a longer query is malformed */
void    rb2_hip_irreducible_dev(rb2_hip_t *h, int64_t n, const uint8_t *qry, const int64_t *off, int64_t max_len, int64_t min_ovlp, int64_t max_ext, int64_t max_steps,
                                int64_t max_recs, int64_t *rec, int64_t *cnt);

/* ---- unitigs: the maximal unbranched paths of a string graph and their texts (csrc/rb2_unitig.h) ----
 * THE GRAPH.  n_str vertices 0 .. n_str-1 and m edges, rows of four int64 src, dst, l, ext (the shape of HipBwt.edges; l is not read).  An
 * edge with src or dst outside [0, n_str) or ext < 1 is IGNORED: counted in info, part of no degree.  outdeg(u) and indeg(v) count the
 * others; a duplicate edge counts twice, a self loop in both degrees.  An edge u -> v is a LINK when outdeg(u) == 1 && indeg(v) == 1, so
 * every vertex has at most one successor and one predecessor through links, and the components of the link relation -- the CHAINS -- are
 * open paths (a lone vertex is a chain of one) and cycles.  The HEAD of an open chain is its vertex without a predecessor; the head of
 * a cycle is its smallest vertex id, and the link into it is the CLOSING LINK.
 * vtx[4v ..] = head, rank, off, ext_in of vertex v: the head of its chain, the links from the head to v, the sum of ext over those
 * links, and ext of the link into v -- -1 for the head of an open chain; for the head of a cycle the ext of the closing link, which is
 * >= 1 and marks the chain as circular.  The closing link is counted in no rank and no off.
 * info = chains, cycles, vertices of the longest chain, edges ignored.  Returns the number of chains.
 * The call does not read the index (n_str is the caller's), waits for a lazy insert and is fatal for n_str or m outside 0 .. 2^36.  Chains
 * are found by pointer jumping: 2 ceil(log2(n_str)) + 5 launches whatever the graph holds, nothing read back between them; 96 bytes of
 * device memory per vertex.  The host variant stages the edges in chunks of 2^24 (RB2_QUERY_CHUNK lowers that) and synchronises once. */
int64_t rb2_hip_unitig_chains(rb2_hip_t *h, int64_t n_str, int64_t m, const int64_t *edges, int64_t *vtx, int64_t info[4]);
/* the same with edges, vtx (4 n_str int64) and info (4 int64) in this device's memory, asynchronous on the handle's stream (no return value: read info) */
void    rb2_hip_unitig_chains_dev(rb2_hip_t *h, int64_t n_str, int64_t m, const int64_t *edges, int64_t *vtx, int64_t *info);
/* THE TEXT of the chains vtx describes, on an index whose string ids are the rows of the `$` block (as for rb2_hip_contained); n_str must
 * equal the number of strings of the index.  The text of the chain with head h and vertices h = v0, v1, .. vk (by rank) is text(v0)
 * followed by the last ext_in(vi) symbols of text(vi) for i = 1 .. k, nt6 codes in text order; its length is len(v0) + off(vk).  If
 * ext_in(vi) > len(vi) (an edge list that does not belong to this index) the piece is the last len(vi) symbols with code 0 in front of
 * them, and the chain is counted in info as one with a SHORT PIECE; every store stays inside the slice of its chain.  A circular chain is
 * cut at its head: the closing link adds nothing.
 * A chain is SELECTED when it has at least min_reads vertices and, with canonical != 0, its smallest vertex id is even: on a graph that
 * is symmetric under v <-> v ^ 1 (strings 2i and 2i + 1 a read and its reverse complement) that keeps exactly one of every unitig and
 * its reverse complement, and a chain that is its own reverse complement once.  The selected chains are numbered by increasing head id:
 * urec[5u ..] = head, n_reads, text_off, text_len, flags of chain u, flags bit 0 = circular, bit 1 = had a short piece; text_off is the
 * exclusive prefix sum of text_len in that order, the text is txt[text_off, text_off + text_len).  A chain is STORED when u < cap_u and
 * text_off + text_len <= cap_txt; the others are counted, and neither their record nor their slice is written (the convention of
 * rb2_hip_kmers' max_recs).  cap_u == 0 or cap_txt == 0 stores nothing and still returns the sizes: that is how a caller sizes urec and txt.
 * info = chains selected, total text length of the selected, selected chains with a short piece, chains stored.  Returns the chains stored.
 * A row of vtx whose head is outside [0, n_str) makes its vertex a chain of its own with the short-piece flag; such a row is followed
 * nowhere, and whatever vtx holds the call stays inside urec, txt and the index (a row whose off or ext_in is negative or above 2^48 adds
 * no piece and flags its chain; sums stop at 2^62).
 * Like every query the call waits for a lazy insert, reads the index and nothing else, and is fatal on one rank of a sharded index; fatal
 * too: n_str < 0 or unequal to the strings of the index, min_reads < 1, a negative cap.  Every vertex that is no head is walked ext_in
 * LF steps, stored or not (that is where a short piece shows); a selected head is walked once for its length and once more when stored. */
int64_t rb2_hip_unitig_text(rb2_hip_t *h, int64_t n_str, const int64_t *vtx, int canonical, int64_t min_reads, int64_t cap_u, int64_t cap_txt, int64_t *urec, uint8_t *txt,
                            int64_t info[4]);
/* the same with vtx, urec (5 cap_u int64) and txt (cap_txt bytes) in this device's memory and info in host memory: the call synchronises
 * the handle's stream once, behind its last kernel, to read the four counts */
int64_t rb2_hip_unitig_text_dev(rb2_hip_t *h, int64_t n_str, const int64_t *vtx, int canonical, int64_t min_reads, int64_t cap_u, int64_t cap_txt, int64_t *urec, uint8_t *txt,
                                int64_t info[4]);

/* 64-bit checksum of rope b computed on the device (position-weighted sum over the packed words of its pieces): equal for
 * equal symbol sequences however the index was built (one engine, N ranks, an .fmr loaded back), sensitive to order.  Lets
 * tests compare indexes of 10^11 symbols without moving them off the device (the reference has no counterpart; its ropes are
 * compared through their .fmd) */
uint64_t rb2_hip_rope_hash(rb2_hip_t *h, int b);

/* ---- the strings of the index, packed, and one index merged into another (csrc/rb2_unpack.h, csrc/rb2_merge_plan.h) ----
 * rb2_hip_unpack[_dev]: the packed inverse BWT of the strings first .. first + n - 1 (ids are rows of the `$` block, as everywhere else).
 * txt[off[i] .. off[i + 1]) holds string first + i followed by one 0 byte, off[0] = 0; an empty string is a lone 0.  reversed != 0: every
 * string LAST symbol first, and txt[0 .. SIZE) is byte for byte a batch rb2_hip_insert_multi[_dev] accepts (each string reversed and
 * 0-terminated); reversed == 0: text order.  Returns SIZE = the sum of the lengths + n.  off (n + 1 values) is written whenever it is
 * not NULL; txt is written only if it is not NULL and cap >= SIZE -- otherwise the call writes NOTHING to txt, not one byte, and still
 * returns SIZE: size with one call, fetch with a second (rb2_hip_save_fmd's convention).  n == 0 returns 0 (off[0] = 0).
 * The _dev variant takes txt and off in device memory; it synchronises the handle's stream ONCE, behind the lengths, to return SIZE
 * (as rb2_hip_unitig_text_dev does), copies the offsets to off and queues the text kernel behind that, asynchronously.  The host variant
 * stages through the query host layer: the lengths in chunks of RB2_QUERY_CHUNK strings, the texts in chunks of at most that many
 * whole strings and 256 MiB of text (one string when it alone is longer), so never more than that is held on the device at once.
 * Like every query both wait for a lazy insert, read the index and nothing else -- layout, sampled suffix array and rope hashes are what
 * they were -- and work on the dense and on the sparse layout.  Cost: two LF walks per string (lengths, then texts); the text walk
 * collects 16 symbols per DPP row and writes them with one store instruction.
 * Fatal, each with a message of its own and before anything is written: one rank of a sharded index; first < 0, n < 0 or first + n above
 * the number of strings; cap < 0; a walk that does not end within N steps or leaves the rows of the index (a loaded index that is no BWT
 * of complete strings).
 *
 * rb2_hip_merge inserts ALL strings of src into dst as rb2_hip_insert_multi_dev would, in dst's own sorting order: the strings go in the
 * order of src's `$` block (in input order string k of src gets the id n_dst + k), in batches of at most batch_bytes bytes of batch
 * text, cut only between strings; a single string longer than the budget is a batch of its own.  The batch is rb2_hip_unpack_dev's
 * reversed output and never leaves the device.  Returns the symbols added, sentinels included.  info (may be NULL) = strings merged,
 * symbols merged without sentinels, batches, bytes of the largest batch.
 * Afterwards dst is byte for byte (rb2_hip_download_rope, rb2_hip_save_fmd, rb2_hip_rope_hash) the index built from dst's strings followed
 * by src's, whatever batch_bytes is: the BWT of a set of strings does not depend on how their insertion is cut into batches, in any
 * sorting order.  src is UNCHANGED (rope hashes, layout, sampled suffix array); dst's sampled suffix array is dropped, as after any insert.
 * An empty src returns 0 and changes nothing; an empty dst ends up holding src's strings, rebuilt in dst's sorting order.
 * batch_bytes == 0 picks a default from rb2_hip_mem_info at the time of the call: a sixteenth of the free device memory, at least 1 MiB
 * and at most 4 GiB; whatever batch_bytes says, a batch holds no more strings than a quarter of the free memory has room for at 128
 * bytes each (the per-string state of an insert; never fewer than 2^20) and no more than the 2^32 - 1024 one batch of the engine may
 * hold.  RB2_MERGE_BATCH in the environment, read on every call, replaces the default (tests).
 * The call returns when dst is complete.  The two handles have streams of their own: the call synchronises src's stream behind every
 * batch text and dst's behind every insert -- two synchronisations per batch, next to those an insert makes anyway.
 * Device memory beyond the two indexes: one batch text, 8 bytes per string of src (the offsets, which never reach the host: it reads
 * 8 bytes per 4096 strings once, and the 4096 offsets around every cut), and what an insert of that batch into dst takes.
 * Fatal, each with a message of its own and before anything is changed: dst == src; handles on different devices; either handle one
 * rank of a sharded index; batch_bytes < 0; a walk in src that does not end (as above). */
int64_t rb2_hip_unpack(rb2_hip_t *h, int64_t first, int64_t n, int reversed, int64_t cap, uint8_t *txt, int64_t *off);
int64_t rb2_hip_unpack_dev(rb2_hip_t *h, int64_t first, int64_t n, int reversed, int64_t cap, uint8_t *txt, int64_t *off);
int64_t rb2_hip_merge(rb2_hip_t *dst, rb2_hip_t *src, int64_t batch_bytes, int64_t info[4]);

/* ---- the string graph of the index's own strings (csrc/rb2_graph.h, csrc/rb2_graph_plan.h) ----
 * The irreducible overlaps of the strings first .. first + n - 1 of the index (the SOURCES; ids are rows of the `$` block, as everywhere
 * else) as an edge list that never leaves the device: rows of four int64 src, dst, l, ext, the shape rb2_hip_unitig_chains reads.
 * For the source s with text S the RECORDS are those rb2_hip_irreducible gives for the query S, under that call's definition and
 * unchanged, with these min_ovlp, max_ext, max_steps and max_recs: have(s) = min(found, max_recs) of them are stored, found following
 * that call's cnt (cnt >= 0: cnt; cnt <= -2, a source that ran out of max_steps: -2 - cnt, and what it found by then is true and is
 * used; a source of more than 8192 symbols has no record and no edge).  The record (l, ext, zlo, zhi) yields min(zhi - zlo, max_hits)
 * EDGES s, dst, l, ext: dst is the string behind the (zlo + k)-th `$`, read from the whole-string table of the sampled suffix array
 * exactly as rb2_hip_string_ids reads it -- the REVERSE COMPLEMENT of the neighbour, as the index yields it -- or, with pairs != 0,
 * that id ^ 1: the neighbour itself on an index whose strings 2i and 2i + 1 are a read and its reverse complement.
 * The rows come in increasing src; the order of the rows of one source is unspecified.  Returns m, the edges of all sources, and stores
 * the first min(m, cap) rows in the order it produces them: every source below the one that is cut is complete, and nothing is written
 * from row cap on.  cap == 0 with edges == NULL counts only: size with one call, fetch with a second.
 * info = m, rows stored, sources that found more than max_recs records, stored records whose range held more than max_hits strings,
 * sources that ran out of max_steps, sources longer than 8192 symbols, 0, 0 (reserved).  n == 0 returns 0 with info zeroed.
 * Cost: per source two LF walks (rb2_hip_unpack's: lengths, texts), the search of rb2_hip_irreducible, and 32 bytes written per edge.
 * The sources are taken in chunks of whole strings: at most RB2_GRAPH_CHUNK strings (in the environment, read on every call; 2^24
 * otherwise and at the most), at most 256 MiB of packed text and at most 256 MiB of records (chunk * max_recs * 32 bytes); a single string
 * is a chunk whatever it takes.  The lengths are known on the device only: a chunk tries a number of strings, the device cuts them at
 * the text budget, and the strings tried and not taken are measured again by the next chunk (a quarter more than fitted is tried then).
 * The host synchronises once per chunk, behind the lengths, and once at the end for info; the rows depend on none of this.
 * Device memory beyond the output: one chunk's text, records and 24 bytes a string, and the stacks of rb2_hip_irreducible (sized for the
 * longest string of the chunk; RB2_IRRED_SCRATCH applies) -- nothing that grows with the index.  The host variant holds cap rows on the
 * device for the time of the call and copies min(m, cap) of them back.
 * Like every query the call waits for a lazy insert, reads the index and nothing else -- layout, rope hashes and the sampled suffix array
 * stay as they were -- and works on the dense and on the sparse layout.  It needs a valid sampled suffix array of any step.
 * Fatal, each with a message of its own and before any launch: no sampled suffix array (call rb2_hip_ssa_build first); one rank of a
 * sharded index; first < 0, n < 0 or first + n above the number of strings; cap < 0, or edges NULL with cap > 0; min_ovlp, max_steps or
 * max_recs below 1, max_ext outside 1 .. 8192 (rb2_hip_irreducible's); max_hits < 1; pairs != 0 on an odd number of strings.  A walk
 * that does not end (a loaded index that is no BWT of complete strings) is fatal as for rb2_hip_unpack. */
int64_t rb2_hip_string_graph(rb2_hip_t *h, int64_t first, int64_t n, int64_t min_ovlp, int64_t max_ext, int64_t max_steps, int64_t max_recs, int64_t max_hits, int pairs,
                             int64_t cap, int64_t *edges, int64_t info[8]);
/* the same with edges (4 cap int64) in this device's memory and info in host memory: what rb2_hip_unitig_chains_dev reads next */
int64_t rb2_hip_string_graph_dev(rb2_hip_t *h, int64_t first, int64_t n, int64_t min_ovlp, int64_t max_ext, int64_t max_steps, int64_t max_recs, int64_t max_hits, int pairs,
                                 int64_t cap, int64_t *edges, int64_t info[8]);

/* ---- tip and bubble removal on an edge list (csrc/rb2_clean.h) ----
 * The step between rb2_hip_string_graph and rb2_hip_unitig_chains: the rows of an edge list that hang short dead ends (TIPS) onto a path
 * or run a short path beside a better one (BUBBLES) are removed, in ROUNDS, and the rows left come back in input order, unchanged.
 * n_str vertices, m rows src, dst, l, ext as rb2_hip_unitig_chains reads them (l is not read, only copied).  No index is read: the handle
 * gives the device and the stream, and like rb2_hip_unitig_chains the call works on any handle, one rank of a sharded index included.
 * VALID ROWS, DEGREES, CHAINS are those of rb2_hip_unitig_chains, exactly: a row with src or dst outside [0, n_str) or ext < 1 is IGNORED
 * (counted, part of nothing, never returned); outdeg and indeg count the other rows still ALIVE, a duplicate twice, a self loop in both;
 * the chains are that call's chains of the rows alive.  Of an open chain c: head(c); tail(c), its vertex of the greatest rank; reads(c),
 * its vertices; minpid(c), the smallest v >> pairs over its vertices (pairs = 1: strings 2i and 2i + 1 are one read, and a chain and its
 * mirror image under v <-> v ^ 1 have the same minpid).  Cycles take part in no rule.
 * A round takes every decision from the rows alive at its start, so nothing depends on an order of evaluation:
 *   OUT-TIP  an open chain with outdeg(tail) == 0, indeg(head) >= 1 and reads <= max_tip_reads.  A row p -> head of an out-tip is removed
 *            iff p has at least one row alive whose dst is not the head of an out-tip (a fork of nothing but short dead ends keeps them all).
 *   IN-TIP   the mirror image: indeg(head) == 0, outdeg(tail) >= 1, reads <= max_tip_reads.  A row tail -> w of an in-tip is removed iff w
 *            has at least one row alive into it whose src is not the tail of an in-tip.
 *   BUBBLE   an open chain is an ARM of (p, q) when indeg(head) == 1 with that row's src = p, outdeg(tail) == 1 with that row's dst = q,
 *            outdeg(p) >= 2 and indeg(q) >= 2.  An arm c LOSES iff reads(c) <= max_bubble_reads and another arm c' of the same (p, q) has
 *            (reads(c'), -minpid(c')) > (reads(c), -minpid(c)) in lexicographic order; the winner may be of any size, and two arms equal
 *            in both keep both.  Both rows of a loser, p -> head and tail -> q, are removed.
 * A row removed by a tip rule counts as a tip row, even when a bubble rule removes it too; any other removed row as a bubble row.  The
 * rounds repeat until one removes nothing or max_rounds have run (a tip that hangs off a tip needs two).  max_tip_reads == 0 or
 * max_bubble_reads == 0 switches that rule off; with both 0 the call is a filter of the ignored rows.
 * Returns m', the rows kept, whatever cap is; row k of them is stored iff k < cap, and nothing is written from row cap on.  cap == 0 with
 * out == NULL counts only.  out must not overlap edges; edges is not written.
 * info = m', rows stored, rounds run (the last one, which found nothing, included), tip rows removed, bubble rows removed, rows ignored,
 * chains of the list as returned (rb2_hip_unitig_chains' info[0] on it), 0.
 * Method: per round k_clean_deg (degrees and the single row into and out of a vertex), the chain launcher of rb2_hip_unitig_chains
 * unchanged, per-head sums (the lanes of a wave that name one head add once), class bits per head, a CSR of the out-rows (the scan of
 * rb2_hip_unitig_text over the out-degrees and an atomic cursor; the order inside a vertex is arbitrary and the rules do not see it), one
 * thread per arm that walks the out-rows of its p -- sum of outdeg(p) over the arms; on a list from rb2_hip_string_graph outdeg is at most
 * max_recs * max_hits --, two anchor bytes per vertex set per row, and one pass that marks the rows removed.  The host synchronises once
 * per round to read that round's counters, and once more for the chains of the result when max_rounds cut the loop; the compaction into
 * out (a keep flag per row, the same scan) is queued behind that, so the _dev variant returns with it in flight on the handle's stream.
 * Device memory beyond the output: 9 bytes per row (a byte that marks the removed rows; 8 for the CSR, then the compaction's scan) and
 * 187 bytes per vertex (96 of the chain launcher, 32 of vtx, 56 per head and degree, 3 flag bytes), plus 8 bytes per 4096 of either.  The
 * host variant also holds the list and min(cap, m) rows of output on the device for the time of the call.
 * Fatal, each with a message of its own, at the top of the call and before any kernel: n_str, m or cap negative or above 2^36; a negative
 * max_tip_reads or max_bubble_reads; max_rounds < 1; pairs outside {0, 1}; edges NULL with m > 0; out NULL with cap > 0; out overlapping
 * edges. */
int64_t rb2_hip_graph_clean(rb2_hip_t *h, int64_t n_str, int64_t m, const int64_t *edges, int64_t max_tip_reads, int64_t max_bubble_reads, int pairs, int64_t max_rounds,
                            int64_t cap, int64_t *out, int64_t info[8]);
/* the same with edges and out (4 cap int64) in this device's memory and info in host memory: what rb2_hip_unitig_chains_dev reads next */
int64_t rb2_hip_graph_clean_dev(rb2_hip_t *h, int64_t n_str, int64_t m, const int64_t *edges, int64_t max_tip_reads, int64_t max_bubble_reads, int pairs, int64_t max_rounds,
                                int64_t cap, int64_t *out, int64_t info[8]);

/* ---- correcting reads by the k-mer spectrum of the index (csrc/rb2_correct.h, csrc/rb2_correct_plan.h) ----
 * The step in front of the overlaps: every exact query stops at the first wrong symbol, so a read with one wrong base loses what lies
 * behind it.  The reads are corrected from the counts of their own k-mers in the index, substitutions only.
 * occ(w) = the occurrences of the word w in the indexed strings: hi - lo of rb2_hip_backward_search on w when the whole word matched
 * (m == k), 0 otherwise; an index of both strands counts both strands.  For a read q of L symbols (nt6 codes 1 .. 5):
 *   WINDOW j (0 <= j <= L - k) is q[j .. j + k).  It is CLEAN when all its symbols are A C G T, SOLID when it is clean and occ >= min_occ.
 *   Position p is WEAK when no solid window contains it.  An N is always weak.
 *   A PROBE is one evaluation of occ on a clean word, and probes are counted; a window that is not clean costs none and is not solid.
 *   Before every probe: if max_probes have been made, the read is OVER BUDGET and stops where it is.
 *   PROFILE: probe the clean windows in increasing j.
 *   LOOP, while fewer than max_fix fixes have been made: stop if no position is weak.  Otherwise go through the weak positions in
 *   increasing p; for each try window ja = max(p - k + 1, 0) (p as far right in it as can be), then jb = min(p, L - k) (as far left; once
 *   only when they are the same window).  A window is tried only if all its symbols other than q[p] are A C G T; trying it means
 *   probing it with b at p for b = A, C, G, T, b != q[p], in that order.  If exactly ONE b is solid: q[p] = b, one FIX, the windows
 *   max(0, p - k + 1) .. min(p, L - k) are evaluated again in increasing j (clean ones probed, the others not solid), and the loop starts
 *   again.  If no weak position yields a fix, stop.
 *   A read with L < k has no window: it comes back as it is with weak = L.
 * Per read: its text with only the fixes changed; cnt >= 0 the fixes; cnt == -1 a malformed read (a code 0 or above 5, more than 8192
 * symbols), its text copied unchanged; cnt <= -2 a read over budget with -2 - cnt fixes made, all of them in the text (a fix whose
 * re-evaluation ran out of probes included); weak = the weak positions at the end, -1 for a malformed read or one over budget.
 * The rule is a heuristic: it restores what a unique solid neighbour restores and may correct to something else where two errors share
 * their windows.  The probe count is fixed by the rule and not by the implementation, so that a model can match budget cases exactly.
 * A probe costs at most k - 1 pairs of ranks: a call ends after n * max_probes * k pairs whatever the index holds.
 * rb2_hip_correct: n reads as for rb2_hip_smem.  out is indexed like qry: out[x] answers qry[x] for x in [off[0], off[n]) and nothing else
 * is written; cnt and weak hold n values each.  Returns the sum of the fixes, those of reads over budget included.  n <= 0 returns 0
 * before the parameters are checked; k, min_occ, max_fix or max_probes below 1 is fatal, each with a message of its own.  The host variant
 * stages chunks of RB2_QUERY_CHUNK reads.  Like every query the call waits for a lazy insert, reads the index and nothing else (layout,
 * rope hashes and a sampled suffix array stay as they were), works on both layouts and is fatal on one rank of a sharded index.
 * One read per 16 lanes (k_correct); the solid bits, one per window, are 1 KiB of LDS per read in flight, so the call sizes nothing from
 * the lengths; at most 2^15 reads are in flight and a row takes further reads a launch apart (RB2_CORRECT_ROWS in the environment, read
 * on every call, lowers the rows: tests). */
int64_t rb2_hip_correct(rb2_hip_t *h, int64_t n, const uint8_t *qry, const int64_t *off, int64_t k, int64_t min_occ, int64_t max_fix, int64_t max_probes, uint8_t *out, int64_t *cnt, int64_t *weak);
/* the same with every pointer in this device's memory, asynchronous on the handle's stream (no return value: read cnt).  total = the
 * caller's bound on off[n] - off[0] (fatal when negative; this implementation keeps the solid bits in LDS and sizes nothing from it).
 * out == qry is allowed: the reads are then corrected where they lie. */
void    rb2_hip_correct_dev(rb2_hip_t *h, int64_t n, const uint8_t *qry, const int64_t *off, int64_t total, int64_t k, int64_t min_occ, int64_t max_fix, int64_t max_probes,
                            uint8_t *out, int64_t *cnt, int64_t *weak);
/* rb2_hip_correct_into corrects EVERY string of src against src and inserts the results into dst without leaving the device: string k of
 * src becomes string n_dst + k in input order.  The batches are cut as rb2_hip_merge cuts them (batch_bytes, its default when 0,
 * RB2_MERGE_BATCH); each is unpacked in text order, corrected into a second buffer, compared, turned round in place (an insert batch
 * holds every string last symbol first and 0-terminated) and inserted.  pairs != 0: strings 2i and 2i + 1 of src are reverse complements
 * of each other (the caller's responsibility, as for rb2_hip_string_graph); only 2i is corrected and 2i + 1 is written as the reverse
 * complement of the result, so dst stays an index of both strands at half the probes; a batch then holds whole pairs.
 * Returns the symbols added, sentinels included.  info (may be NULL) = strings, strings whose text changed, fixes, strings left with a
 * weak position, strings over budget, malformed strings (longer than 8192 symbols: copied as they are), batches, bytes of the largest
 * batch; with pairs the four counts in the middle and the changed strings count the strings 2i only.
 * src is UNCHANGED (rope hashes, layout, sampled suffix array); dst's sampled suffix array is dropped, as after any insert.  Device
 * memory beyond the two indexes: two batch texts, 8 bytes per string of src and 16 per corrected string of a batch.
 * Fatal, each with a message of its own and before anything is changed: dst == src; handles on different devices; either handle one rank
 * of a sharded index; batch_bytes < 0; k, min_occ, max_fix or max_probes below 1; pairs != 0 on an odd number of strings. */
int64_t rb2_hip_correct_into(rb2_hip_t *dst, rb2_hip_t *src, int64_t k, int64_t min_occ, int64_t max_fix, int64_t max_probes, int pairs, int64_t batch_bytes, int64_t info[8]);

/* ---- rope sharding across GPUs ---------------------------------------------------------------
 * The unit of ownership is a SUB-ROPE: rope b is kept as six independent pieces (b,x), x = the symbol that follows b in the
 * row's suffix (piece (b,x) holds exactly the b-symbols of rope x; rope $ is one piece; NR = 31 pieces, see rb2_device.h).
 * owner[r] = rank that holds piece r and processes its bucket.  Inside a round the pieces are independent (the reference runs
 * the ropes on separate threads, mrope.c:312-329); between rounds every rank needs the NR x 6 count matrix (the master reads
 * r[b]->c[] of all ropes, mrope.c:332-340) and strings move from piece (b,x) to the owner of piece (a,b) for the symbol a they
 * just inserted (mrope.c:303-309).  Both exchanges happen inside the library: rb2_hip_multi_* below.  (Rounds 2-3 also exported
 * the phases of a round one by one, rb2_hip_shard_*, for a Python driver that issued the collectives itself; that second
 * protocol was retired in round 4.) */
int     rb2_hip_num_subropes(void);                    /* NR = 31: rope $ + pieces (b,x), index 1+(b-1)*6+x */
void    rb2_hip_memcpy(rb2_hip_t *h, void *dst, const void *src, int64_t bytes, int kind);   /* on the handle's stream; kind 0 host->device, 1 device->host, 2 device->device */
/* run on the caller's stream (e.g. torch.cuda.current_stream().cuda_stream): the caller's own work on that stream and the
 * engine's kernels then need no host synchronisation between them */
void    rb2_hip_use_stream(rb2_hip_t *h, void *hip_stream);


/* ---- N GPUs behind one handle (round 3) ------------------------------------------------------------------
 * The reference fans a round out to its workers and joins them INSIDE mr_insert_multi (mrope.c:287-296, 312-329) and reads
 * every rope's counts after the barrier (mrope.c:332-340); callers just call mr_insert_multi (main.c:240, 248).  This is the
 * same contract for N engines: one call inserts a batch into ONE index whose 31 sub-ropes are dealt out over the ranks
 * (owner map: owner[r] = rank of sub-rope r), the round loop -- count matrix, merge, exchange of the string records, unpack --
 * runs inside the library, one host thread per local rank, no host <-> device synchronisation between the rounds of a
 * batch on the PEER transport.  Two transports behind the same loop:
 *   RB2_TRANSPORT_PEER  one process, every rank an engine of its own on devices[i] (the same device may be listed several
 *                       times: N "virtual" ranks on one GPU -- how the whole path is tested on a one-GPU box).  The count
 *                       matrices are summed by a kernel that reads the peers' rows, the string records are fetched by the
 *                       RECEIVER's unpack kernel straight from the senders' buffers (peer access over xGMI; device events
 *                       order the streams), so an exchange costs no launch of its own and no host round trip.
 *   RB2_TRANSPORT_RCCL  RCCL's C API (librccl, loaded on first use): ncclAllReduce of the 31 x 6 matrix in place, grouped
 *                       ncclSend / ncclRecv of the records.  Works across processes (rb2_hip_multi_create_rank: one process
 *                       per GPU, the launch contract of bench.py) and inside one (rb2_hip_multi_create on distinct devices).
 *                       The host reads the reduced matrix from pinned memory behind an event that fires BEFORE the merge
 *                       kernels of the round run -- it sizes the sends while the GPU merges; the stream never drains.
 */
typedef struct rb2_hip_multi_s rb2_hip_multi_t;
#define RB2_TRANSPORT_PEER 0
#define RB2_TRANSPORT_RCCL 1
#define RB2_MULTI_MAX_RANKS 64
/* one process drives n ranks; devices[i] = HIP device of rank i; owner == NULL: the default owner map (rb2_hip_default_owners) */
/* Start-up checks (round 4), so that the first run on real multi-GPU hardware fails loudly or not at all:
 *   - PEER transport asked for, but some pair of the listed devices has no peer access: the handle is created on the RCCL
 *     transport instead (message on stderr; never a CPU path).  Impossible (a device listed twice AND a pair without peer access): fatal.
 *   - self-test: whenever the ranks sit on more than one physical device (or RB2_MULTI_SELFTEST=1; =0 turns it off) a job of
 *     2000 short reads is built across the ranks and, sub-rope by sub-rope, compared -- device-side checksums and the count matrix
 *     -- with the same job on one engine; a mismatch is fatal.  The handle is reset afterwards.  Under rb2_hip_multi_create_rank (one
 *     process per GPU) the self-test is a COLLECTIVE: every process of the group must take the same decision, i.e. RB2_MULTI_SELFTEST
 *     must be set to the same value (or left unset) in all of them -- a rank that skips it alone leaves the others waiting in RCCL. */
rb2_hip_multi_t *rb2_hip_multi_create(int n, const int *devices, int sorting_order, int transport, const int *owner /* [NR] or NULL */);
/* the transport the handle really uses (RB2_TRANSPORT_*) */
int rb2_hip_multi_transport(const rb2_hip_multi_t *m);
/* one rank of a group of `nranks` processes (RCCL): `nccl_id` = the 128 bytes rb2_hip_multi_unique_id() produced on rank 0 */
void rb2_hip_multi_unique_id(void *id128);
rb2_hip_multi_t *rb2_hip_multi_create_rank(int device, int rank, int nranks, const void *nccl_id, int sorting_order, const int *owner);
void rb2_hip_multi_destroy(rb2_hip_multi_t *m);
void rb2_hip_default_owners(int nranks, int owner[] /* NR */);
int  rb2_hip_multi_nranks(const rb2_hip_multi_t *m);            /* ranks of the whole group */
int  rb2_hip_multi_nlocal(const rb2_hip_multi_t *m);            /* ... driven by this process */
rb2_hip_t *rb2_hip_multi_engine(rb2_hip_multi_t *m, int local_rank);   /* the engine of a local rank (profiling, rb2_hip_dev_alloc, ...) */
/* mr_insert_multi (mrope.c:258) on the sharded index: `s` host memory, borrowed for the call (uploaded once per device) */
void rb2_hip_multi_insert_multi(rb2_hip_multi_t *m, int64_t len, const uint8_t *s);
/* the batch already sits on the devices: s_dev[i] = the (whole) batch text in the memory of local rank i's device, 16-byte
 * aligned; ranks on one device may share a buffer */
void rb2_hip_multi_insert_multi_dev(rb2_hip_multi_t *m, int64_t len, const uint8_t *const *s_dev);
void rb2_hip_multi_get_counts(rb2_hip_multi_t *m, int64_t c[36]);
/* rope b as run bytes: its pieces (b,x), x = $ACGTN, each from its owner, in order.  A multi-process handle only holds the
 * pieces of its own rank: the functions then return those (in order) -- gathering across processes is the caller's job */
int64_t rb2_hip_multi_rope_bytes(rb2_hip_multi_t *m, int b);
int64_t rb2_hip_multi_download_rope(rb2_hip_multi_t *m, int b, uint8_t *dst);
int64_t rb2_hip_multi_stream_rope(rb2_hip_multi_t *m, int b, rb2_hip_run_cb cb, void *user);
void rb2_hip_multi_load_ropes(rb2_hip_multi_t *m, const uint8_t *const rle[6], const int64_t n_bytes[6]);
/* rb2_hip_load_fmd on the sharded index: every rank decodes the stream and keeps its own pieces */
int64_t rb2_hip_multi_load_fmd(rb2_hip_multi_t *m, const void *fmd, int64_t n_bytes);
void rb2_hip_multi_reserve(rb2_hip_multi_t *m, int64_t batch_bytes, int64_t batch_strings, int64_t total_symbols);
void rb2_hip_multi_reset(rb2_hip_multi_t *m);
void rb2_hip_multi_sync(rb2_hip_multi_t *m);
void rb2_hip_multi_rank1a(rb2_hip_multi_t *m, int b, int64_t x, int64_t cx[6]);
/* out[0] host <-> device synchronisations inside the round loops so far (PEER: none in dense rounds; an in-place round reads a
 * one-word verdict before its exchange; RCCL: one event wait per round, behind the reduce only), out[1] rounds, out[2] batches,
 * out[3] in-place (sparse) rounds summed over the ranks, out[4] void sparse rounds, out[5] re-layouts */
void rb2_hip_multi_stats(rb2_hip_multi_t *m, int64_t out[6]);
/* bytes of device memory local rank k holds for the text of the last batch given to rb2_hip_multi_insert_multi (host buffer): with
 * ranks on several devices of one process (PEER) the text is ONE copy, shared piece by piece between the devices' memories and
 * mapped for all of them -- about len / n per rank, each rank uploads its own share --, otherwise a copy of the whole batch per
 * device, held by the first rank on it (0 for the others); -1: no such rank.  RB2_MULTI_TEXT=shard / =copy forces either. */
int64_t rb2_hip_multi_text_bytes(const rb2_hip_multi_t *m, int k);
uint64_t rb2_hip_multi_rope_hash(rb2_hip_multi_t *m, int b);
/* the device-side exchange plan (k_mround) evaluated on the host, for tests: see csrc/rb2_multi.h */
int rb2_hip_multi_plan_host(const int *owner /* [NR] */, int nranks, const int64_t *g /* [NR*6] */, int me, int64_t *sdest /* [NR*6] */, int64_t (*pieces)[5] /* [NR*6] */, int64_t *total);   /* == rb2_hip_rope_hash of the same rope on one engine */

/* ---- measurement helpers (bench.py; not part of the reference API) ------------------------ */

/* allocate / free raw device memory */
void *rb2_hip_dev_alloc(rb2_hip_t *h, int64_t bytes);
void  rb2_hip_dev_free(rb2_hip_t *h, void *p);

/* fill dst_dev (n_reads*(read_len+1) bytes) with synthetic reads first_read..first_read+n_reads
 * of the SURVEY.md 8c generator (splitmix64 counter stream), already nt6-encoded, reversed and
 * 0-terminated -- i.e. exactly what main.c:177-237 would put in the batch buffer for `-R`.
 * strand: 0 = forward strand only; 1 = forward followed by reverse complement (buffer doubles). */
void rb2_hip_synth_reads(rb2_hip_t *h, uint8_t *dst_dev, int64_t first_read, int64_t n_reads,
                         int read_len, uint64_t seed, int strand);
/* the same, but the reads are windows of one random genome of genome_len bases (uniform start positions): overlapping
 * reads as from sequencing at coverage n_reads*read_len/genome_len -- large groups, non-empty intervals in every round */
void rb2_hip_synth_reads_cov(rb2_hip_t *h, uint8_t *dst_dev, int64_t first_read, int64_t n_reads,
                             int read_len, uint64_t seed, int strand, int64_t genome_len);
/* ... with a composition knob: skew != 0 draws 85 % A and 5 % each of C, G, T from the same random words (tools/synth_reads.c,
 * seventh argument): sub-rope (A,A) then holds 72 % of the index and passes 2^32 symbols at 59 M x 101 bp */
void rb2_hip_synth_reads_skew(rb2_hip_t *h, uint8_t *dst_dev, int64_t first_read, int64_t n_reads,
                              int read_len, uint64_t seed, int strand, int64_t genome_len, int skew);

void rb2_hip_sync(rb2_hip_t *h);

/* leaf-layout statistics since rb2_hip_create: out[0] re-layouts (dense <-> sparse), out[1] void sparse rounds (a leaf ran out
 * of slack; the round was redone densely), out[2] rounds inserted in place, out[3] 1 when the index currently has the sparse layout */
void rb2_hip_sparse_stats(rb2_hip_t *h, int64_t out[4]);
/* the same four, then out[4] re-spreads among the re-layouts (sparse -> sparse: a superblock had no free slot for a split),
 * out[5] leaves split in place by k_split (the leaf split of rope.c:143-146); out[6] device buffers that had to grow while the rounds
 * of a dense batch were being queued (each one is a device-wide wait in the middle of the batch: 0 unless a sizing rule is missing);
 * out[7] reserved */
void rb2_hip_layout_stats(rb2_hip_t *h, int64_t out[8]);
/* void in-place rounds the host took back from behind the rounds it had queued after them (one engine queues in-place rounds without
 * waiting for their verdict; a void round makes every kernel behind it return, and the host rewinds its own bookkeeping when it finds
 * out): out[0] such rewinds, out[1] queued rounds taken back in all (the void round included: depth = rounds queued from it on),
 * out[2] the deepest rewind, out[3] rewinds of even depth (the descriptor and array sides stay where they are).  Every void round
 * of a single-engine insert is counted here unless RB2_LAZY_VERDICT=0; RB2_VERDICT_POLL=0 (tests) defers the host's look at the
 * verdict to the next drain, which makes rewinds deep. */
void rb2_hip_rewind_stats(rb2_hip_t *h, int64_t out[4]);
/* rounds of one-member groups (a single engine): the device reports, without a synchronisation, the first round of a batch in
 * which every interval was empty and every string a group of its own; from then on the host knows every interval empty and the dense rounds
 * launch no k_prep.  out[0] = 0 (dense rounds launched with a k_advance instantiation of their own: measured, no gain, not part of the library),
 * out[1] = dense rounds without a k_prep<AE> launch since create, out[2] = round of the last batch at which the device first reported the
 * state (-1: never), out[3] = round of the last batch from which the host used it (-1: never).  RB2_STEADY=0 at create keeps the k_prep<AE>
 * launch of every round (the report is still read);
 * RB2_STEADY_AHEAD=n (default 3, 0: no bound) is how many rounds an insert that is waited for may queue ahead of the last round reported until
 * the state is reached or 48 rounds of the batch are queued. */
void rb2_hip_steady_stats(rb2_hip_t *h, int64_t out[4]);
/* lean rounds ("the lean round"): a dense round of a single engine that the host knows to be one of one-member groups and empty
 * intervals when it queues its counting phase writes no insert list (INS_E / INS_A); the window search and the merge read the strings' positions and
 * symbols in its place.  out[0] = dense rounds run lean since create, out[1] = the stage in force: 0 = off, 1 = no insert list, 2 = no insert list and
 * the round is counted from the symbols alone (RB2_STEADY_LEAN=0 / 1 / 2 at create; a larger value means 2; RB2_STEADY=0 switches it off as well).
 * Stage 2 takes the lean rounds whose counting tail is the three-launch form only: a handle created with it reports 1 until it has queued such a
 * round (batches of few string tiles never do: their lean rounds are stage-1 rounds), 2 from then on. */
void rb2_hip_lean_stats(rb2_hip_t *h, int64_t out[2]);
/* stage 2 of the lean round ("the lean count"): one small launch (k_count_lean) writes the tile records and chunk totals of
 * the round from the strings' symbols, in the place of the k_sym and k_tscan1 launches.  out[0] = rounds counted that way since create, out[1] =
 * audit rounds (every RB2_LEAN_AUDIT-th lean round of a batch, default 8, 0 = never, is counted by k_sym as in stage 1: it looks at the positions
 * and keeps the guard of the steady round alive), out[2] = rounds in which both ways ran and were compared (RB2_LEAN_VERIFY=1 at create; tests),
 * out[3] = words in which they differed (a difference is fatal at the end of its batch). */
void rb2_hip_lean_count_stats(rb2_hip_t *h, int64_t out[4]);
/* the forked round ("the forked round"): the counting tail of a round counted by k_count_lean runs on a side stream of the handle's
 * own, beside the window search, the merge and the directory of the same round, which need the bucket sizes only; k_advance waits for both.
 * out[0] = rounds forked since create, out[1] = 1 when such rounds are forked (RB2_LEAN_FORK, default 1; 0 at create: one stream, the launches as
 * before), 0 when not -- the switch is off, the handle runs on a caller's stream (rb2_hip_use_stream), or RB2_LEAN_VERIFY / RB2_HIP_DEBUG is set. */
void rb2_hip_lean_fork_stats(rb2_hip_t *h, int64_t out[2]);
/* the window directory ("the window directory"): a lean round whose windows may be written compact keeps the rank directory of the
 * side it writes per window of 4 leaves, not per leaf -- nothing but the merge and the round's own k_advance reads that side before the next rewrite.
 * out[0] = rounds run that way since create, out[1] = the switch (RB2_LEAN_DIR, default 1; 0 at create: every round writes the per-leaf
 * directory, the launches as before), out[2] = the rounds the mode applies to, counted whatever the switch says: the lean rounds among the rounds
 * rb2_hip_window_stats counts in out[4]. */
void rb2_hip_lean_dir_stats(rb2_hip_t *h, int64_t out[3]);
/* window formats of the dense layout (a window = 4 leaves = 4096 symbols; csrc/rb2_merge.h): out[0..3] = windows the dense merge wrote
 * plain (three bit planes) / compact with no, one, two lines of exception positions -- counted on the device only when the handle was
 * created with RB2_COMPACT_STATS=1 in the environment (zeros otherwise) --, out[4] = dense rounds that were allowed to write compact
 * windows (all intervals empty, not the last round of a batch, no re-layout ahead), out[5] = 1 when the per-format counts are on.
 * RB2_COMPACT=0 keeps every window plain.  The reference has no counterpart: its leaves are always run-length coded (rle.h:39-75). */
void rb2_hip_window_stats(rb2_hip_t *h, int64_t out[6]);

/* per-kernel timing, measured with hipEvents on the engine's own stream when enabled */
#define RB2_K_SYM      0
#define RB2_K_TSCAN    1
#define RB2_K_PREP     2
#define RB2_K_PART     3
#define RB2_K_MERGE    4
#define RB2_K_META     5
#define RB2_K_ADVANCE  6
#define RB2_K_INIT     7
#define RB2_K_RELAYOUT 8   /* change between the dense and the sparse (slack) leaf layout */
#define RB2_K_SPLIT    9   /* leaf splits at the end of an in-place round */
#define RB2_K_COUNT    10
void rb2_hip_profile(rb2_hip_t *h, int enable);   /* 0: off; 1: every kernel group of a round (sixteen events per round); 2: the merge launches only (two) */
/* launches[k], ms[k] (summed), units[k] (strings processed, summed) since the last reset */
void rb2_hip_profile_get(rb2_hip_t *h, int64_t launches[RB2_K_COUNT], double ms[RB2_K_COUNT],
                         int64_t units[RB2_K_COUNT], int reset);
const char *rb2_hip_kernel_name(int k);

/* device layout constants: symbols per leaf, leaves per merge tile, strings per string tile */
void rb2_hip_layout(int *leaf_syms, int *tile_leaves, int *string_tile);

/* diagnostic: one of the engine's cold-path prefix scans (rb2_scan.h) over the host array in[0 .. n), run in place on the device.
 * op 0: sums of uint32 (in[] is narrowed), 1: sums of uint64, 2: sums that stop at 2^62, an item counting as 2^62 at the most,
 * 3: running maximum.  out[i], i < n: the items in front of i (op 3: up to and including i); out[n] and *total: all of them.
 * form 0: many blocks in three launches, and parts[b] = the items in front of block b, for every block that holds an item;
 * form 1 / 2: one block of 256 / 1024 threads (op 1 only; parts is not written).  Returns the items a block takes per turn.
 * One synchronise. */
int64_t rb2_hip_scan_check(rb2_hip_t *h, int op, int form, int64_t n, const uint64_t *in, uint64_t *out, uint64_t *parts, uint64_t *total);

#ifdef __cplusplus
}
#endif
#endif
