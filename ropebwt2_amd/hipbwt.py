"""ctypes mirror of include/rb2_hip.h -- the C ABI of the gfx950 insertion engine.

``HipBwt`` follows the reference's operator interface for this path: ``insert_multi(buf)`` takes
exactly the buffer main.c hands to ``mr_insert_multi`` (mrope.h:46-54: concatenated, reversed,
0-terminated nt6 strings) and mutates the six ropes; ``counts()`` is ``rope_t.c`` (rope.h:19).
"""
import ctypes as C
import os

import numpy as np

from .build import lib_path

K_NAMES = ["k_sym", "k_tscan", "k_prep", "k_part", "k_merge", "k_meta", "k_advance", "k_init", "k_relayout", "k_split"]
_lib = None


def load_hip_lib():
    """Load librb2hip.so; raises (never falls back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("RB2_HIP_LIB") or lib_path("librb2hip.so")      # (RB2_HIP_LIB: A/B runs of two builds on one box)
    if not os.path.exists(path):
        raise RuntimeError("%s missing: run `python -m ropebwt2_amd.build` (hipcc, gfx950) first" % path)
    L = C.CDLL(path)
    vp, i64, i32, u64 = C.c_void_p, C.c_int64, C.c_int, C.c_uint64
    sig = {
        "rb2_hip_device_count": (i32, []),
        "rb2_hip_set_fatal_handler": (None, [vp, vp]),
        "rb2_hip_create": (vp, [i32, i32]),
        "rb2_hip_destroy": (None, [vp]),
        "rb2_hip_sorting_order": (i32, [vp]),
        "rb2_hip_reset": (None, [vp]),
        "rb2_hip_insert_multi": (None, [vp, i64, vp]),
        "rb2_hip_insert_multi_dev": (None, [vp, i64, vp]),
        "rb2_hip_prefetch": (None, [vp, vp, i64, i64]),
        "rb2_hip_set_lazy": (None, [vp, C.c_int]),
        "rb2_hip_wait": (None, [vp]),
        "rb2_hip_last_batch_counts": (C.c_int, [vp, vp]),
        "rb2_hip_mem_info": (None, [i32, vp, vp]),
        "rb2_hip_get_counts": (None, [vp, vp]),
        "rb2_hip_rope_bytes": (i64, [vp, i32]),
        "rb2_hip_download_rope": (i64, [vp, i32, vp]),
        "rb2_hip_stream_rope": (i64, [vp, i32, vp, vp]),
        "rb2_hip_load_ropes": (None, [vp, vp, vp]),
        "rb2_hip_load_fmd": (i64, [vp, vp, i64]),
        "rb2_hip_load_fmd_file": (i64, [vp, C.c_char_p]),
        "rb2_hip_save_fmd": (i64, [vp, vp, i64]),
        "rb2_hip_save_fmd_file": (i64, [vp, C.c_char_p]),
        "rb2_hip_delete_strings": (i64, [vp, i64, vp]),
        "rb2_hip_delete_stats": (None, [vp, vp]),
        "rb2_hip_rank1a": (None, [vp, i32, i64, vp]),
        "rb2_hip_rank_batch": (None, [vp, i32, i64, vp, vp]),
        "rb2_hip_backward_search": (None, [vp, i64, vp, vp, vp]),
        "rb2_hip_backward_search_dev": (None, [vp, i64, vp, vp, vp]),
        "rb2_hip_extend": (None, [vp, i64, vp, i32, vp]),
        "rb2_hip_extract": (i64, [vp, i64, vp, i64, vp, vp]),
        "rb2_hip_smem": (i64, [vp, i64, vp, vp, i64, i64, i64, vp, vp]),
        "rb2_hip_smem_dev": (None, [vp, i64, vp, vp, i64, i64, i64, vp, vp]),
        "rb2_hip_ssa_build": (i64, [vp, i32]),
        "rb2_hip_ssa_drop": (None, [vp]),
        "rb2_hip_ssa_info": (None, [vp, vp]),
        "rb2_hip_locate": (i64, [vp, i64, vp, i64, vp, vp]),
        "rb2_hip_locate_dev": (None, [vp, i64, vp, i64, vp, vp]),
        "rb2_hip_overlap": (i64, [vp, i64, vp, vp, i64, i64, vp, vp]),
        "rb2_hip_overlap_dev": (None, [vp, i64, vp, vp, i64, i64, vp, vp]),
        "rb2_hip_string_ids": (i64, [vp, i64, vp, i64, vp, vp]),
        "rb2_hip_string_ids_dev": (None, [vp, i64, vp, i64, vp, vp]),
        "rb2_hip_kmers": (i64, [vp, i32, i64, i32, i64, vp, i64, vp, vp]),
        "rb2_hip_approx": (i64, [vp, i64, vp, vp, i32, i64, i64, i64, vp, vp]),
        "rb2_hip_approx_dev": (None, [vp, i64, vp, vp, i32, i64, i64, i64, vp, vp]),
        "rb2_hip_approx_ed": (i64, [vp, i64, vp, vp, i32, i64, i64, i64, vp, vp]),
        "rb2_hip_approx_ed_dev": (None, [vp, i64, vp, vp, i32, i64, i64, i64, vp, vp]),
        "rb2_hip_contained": (i64, [vp, i64, vp, vp]),
        "rb2_hip_contained_dev": (None, [vp, i64, vp, vp]),
        "rb2_hip_irreducible": (i64, [vp, i64, vp, vp, i64, i64, i64, i64, vp, vp]),
        "rb2_hip_irreducible_dev": (None, [vp, i64, vp, vp, i64, i64, i64, i64, i64, vp, vp]),
        "rb2_hip_unitig_chains": (i64, [vp, i64, i64, vp, vp, vp]),
        "rb2_hip_unitig_chains_dev": (None, [vp, i64, i64, vp, vp, vp]),
        "rb2_hip_unitig_text": (i64, [vp, i64, vp, i32, i64, i64, i64, vp, vp, vp]),
        "rb2_hip_unitig_text_dev": (i64, [vp, i64, vp, i32, i64, i64, i64, vp, vp, vp]),
        "rb2_hip_unpack": (i64, [vp, i64, i64, i32, i64, vp, vp]),
        "rb2_hip_unpack_dev": (i64, [vp, i64, i64, i32, i64, vp, vp]),
        "rb2_hip_merge": (i64, [vp, vp, i64, vp]),
        "rb2_hip_string_graph": (i64, [vp, i64, i64, i64, i64, i64, i64, i64, i32, i64, vp, vp]),
        "rb2_hip_string_graph_dev": (i64, [vp, i64, i64, i64, i64, i64, i64, i64, i32, i64, vp, vp]),
        "rb2_hip_graph_clean": (i64, [vp, i64, i64, vp, i64, i64, i32, i64, i64, vp, vp]),
        "rb2_hip_graph_clean_dev": (i64, [vp, i64, i64, vp, i64, i64, i32, i64, i64, vp, vp]),
        "rb2_hip_correct": (i64, [vp, i64, vp, vp, i64, i64, i64, i64, vp, vp, vp]),
        "rb2_hip_correct_dev": (None, [vp, i64, vp, vp, i64, i64, i64, i64, i64, vp, vp, vp]),
        "rb2_hip_correct_into": (i64, [vp, vp, i64, i64, i64, i64, i32, i64, vp]),
        "rb2_hip_reserve": (None, [vp, i64, i64, i64]),
        "rb2_hip_num_subropes": (i32, []),
        "rb2_hip_memcpy": (None, [vp, vp, vp, i64, i32]),
        "rb2_hip_use_stream": (None, [vp, vp]),
        "rb2_hip_dev_alloc": (vp, [vp, i64]),
        "rb2_hip_dev_free": (None, [vp, vp]),
        "rb2_hip_synth_reads": (None, [vp, vp, i64, i64, i32, u64, i32]),
        "rb2_hip_synth_reads_cov": (None, [vp, vp, i64, i64, i32, u64, i32, i64]),
        "rb2_hip_synth_reads_skew": (None, [vp, vp, i64, i64, i32, u64, i32, i64, i32]),
        "rb2_hip_sync": (None, [vp]),
        "rb2_hip_sparse_stats": (None, [vp, vp]),
        "rb2_hip_layout_stats": (None, [vp, vp]),
        "rb2_hip_rewind_stats": (None, [vp, vp]),
        "rb2_hip_steady_stats": (None, [vp, vp]),
        "rb2_hip_lean_stats": (None, [vp, vp]),
        "rb2_hip_lean_count_stats": (None, [vp, vp]),
        "rb2_hip_lean_fork_stats": (None, [vp, vp]),
        "rb2_hip_lean_dir_stats": (None, [vp, vp]),
        "rb2_hip_window_stats": (None, [vp, vp]),
        "rb2_hip_host_register": (C.c_int, [vp, C.c_int64]),
        "rb2_hip_host_unregister": (C.c_int, [vp]),
        "rb2_hip_profile": (None, [vp, i32]),
        "rb2_hip_profile_get": (None, [vp, vp, vp, vp, i32]),
        "rb2_hip_kernel_name": (C.c_char_p, [i32]),
        "rb2_hip_layout": (None, [vp, vp, vp]),
        "rb2_hip_scan_check": (i64, [vp, i32, i32, i64, vp, vp, vp, vp]),
        "rb2_hip_multi_create": (vp, [i32, vp, i32, i32, vp]),
        "rb2_hip_multi_unique_id": (None, [vp]),
        "rb2_hip_multi_create_rank": (vp, [i32, i32, i32, vp, i32, vp]),
        "rb2_hip_multi_destroy": (None, [vp]),
        "rb2_hip_default_owners": (None, [i32, vp]),
        "rb2_hip_multi_nranks": (i32, [vp]),
        "rb2_hip_multi_transport": (i32, [vp]),
        "rb2_hip_multi_nlocal": (i32, [vp]),
        "rb2_hip_multi_engine": (vp, [vp, i32]),
        "rb2_hip_multi_insert_multi": (None, [vp, i64, vp]),
        "rb2_hip_multi_insert_multi_dev": (None, [vp, i64, vp]),
        "rb2_hip_multi_get_counts": (None, [vp, vp]),
        "rb2_hip_multi_rope_bytes": (i64, [vp, i32]),
        "rb2_hip_multi_download_rope": (i64, [vp, i32, vp]),
        "rb2_hip_multi_stream_rope": (i64, [vp, i32, vp, vp]),
        "rb2_hip_multi_load_ropes": (None, [vp, vp, vp]),
        "rb2_hip_multi_load_fmd": (i64, [vp, vp, i64]),
        "rb2_hip_multi_reserve": (None, [vp, i64, i64, i64]),
        "rb2_hip_multi_reset": (None, [vp]),
        "rb2_hip_multi_sync": (None, [vp]),
        "rb2_hip_multi_rank1a": (None, [vp, i32, i64, vp]),
        "rb2_hip_multi_stats": (None, [vp, vp]),
        "rb2_hip_multi_text_bytes": (i64, [vp, C.c_int]),
        "rb2_hip_multi_rope_hash": (u64, [vp, i32]),
        "rb2_hip_multi_plan_host": (i32, [vp, i32, vp, i32, vp, vp, vp]),
        "rb2_hip_rope_hash": (u64, [vp, i32]),
    }
    for name, (res, args) in sig.items():
        try:
            f = getattr(L, name)
        except AttributeError:
            if os.environ.get("RB2_HIP_LIB"):                  # an older build in an A/B run: what it lacks is simply not callable
                continue
            raise
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


ABI_SYMBOLS = [
    "rb2_hip_device_count", "rb2_hip_set_fatal_handler", "rb2_hip_create", "rb2_hip_destroy", "rb2_hip_sorting_order", "rb2_hip_reset",
    "rb2_hip_insert_multi", "rb2_hip_insert_multi_dev", "rb2_hip_set_lazy", "rb2_hip_wait", "rb2_hip_last_batch_counts", "rb2_hip_prefetch", "rb2_hip_mem_info", "rb2_hip_get_counts", "rb2_hip_rope_bytes",
    "rb2_hip_download_rope", "rb2_hip_stream_rope", "rb2_hip_load_ropes", "rb2_hip_load_fmd", "rb2_hip_load_fmd_file", "rb2_hip_save_fmd", "rb2_hip_save_fmd_file", "rb2_hip_delete_strings", "rb2_hip_delete_stats", "rb2_hip_rank1a", "rb2_hip_rank_batch", "rb2_hip_reserve",
    "rb2_hip_backward_search", "rb2_hip_backward_search_dev", "rb2_hip_extend", "rb2_hip_extract", "rb2_hip_smem", "rb2_hip_smem_dev", "rb2_hip_dev_alloc",
    "rb2_hip_ssa_build", "rb2_hip_ssa_drop", "rb2_hip_ssa_info", "rb2_hip_locate", "rb2_hip_locate_dev",
    "rb2_hip_overlap", "rb2_hip_overlap_dev", "rb2_hip_string_ids", "rb2_hip_string_ids_dev", "rb2_hip_kmers",
    "rb2_hip_approx", "rb2_hip_approx_dev", "rb2_hip_approx_ed", "rb2_hip_approx_ed_dev", "rb2_hip_contained", "rb2_hip_contained_dev",
    "rb2_hip_irreducible", "rb2_hip_irreducible_dev",
    "rb2_hip_unitig_chains", "rb2_hip_unitig_chains_dev", "rb2_hip_unitig_text", "rb2_hip_unitig_text_dev",
    "rb2_hip_unpack", "rb2_hip_unpack_dev", "rb2_hip_merge",
    "rb2_hip_string_graph", "rb2_hip_string_graph_dev", "rb2_hip_graph_clean", "rb2_hip_graph_clean_dev",
    "rb2_hip_correct", "rb2_hip_correct_dev", "rb2_hip_correct_into",
    "rb2_hip_num_subropes", "rb2_hip_memcpy", "rb2_hip_use_stream",
    "rb2_hip_dev_free", "rb2_hip_synth_reads", "rb2_hip_synth_reads_cov", "rb2_hip_synth_reads_skew", "rb2_hip_sync", "rb2_hip_sparse_stats", "rb2_hip_layout_stats", "rb2_hip_rewind_stats", "rb2_hip_steady_stats", "rb2_hip_lean_stats", "rb2_hip_lean_count_stats", "rb2_hip_lean_fork_stats", "rb2_hip_lean_dir_stats", "rb2_hip_window_stats", "rb2_hip_host_register", "rb2_hip_host_unregister", "rb2_hip_profile",
    "rb2_hip_profile_get", "rb2_hip_kernel_name", "rb2_hip_layout", "rb2_hip_scan_check",
    "rb2_hip_multi_create", "rb2_hip_multi_unique_id", "rb2_hip_multi_create_rank", "rb2_hip_multi_destroy", "rb2_hip_default_owners",
    "rb2_hip_multi_nranks", "rb2_hip_multi_transport", "rb2_hip_multi_nlocal", "rb2_hip_multi_engine", "rb2_hip_multi_insert_multi", "rb2_hip_multi_insert_multi_dev",
    "rb2_hip_multi_get_counts", "rb2_hip_multi_rope_bytes", "rb2_hip_multi_download_rope", "rb2_hip_multi_stream_rope",
    "rb2_hip_multi_load_ropes", "rb2_hip_multi_load_fmd", "rb2_hip_multi_reserve", "rb2_hip_multi_rope_hash", "rb2_hip_rope_hash", "rb2_hip_multi_plan_host", "rb2_hip_multi_reset", "rb2_hip_multi_sync", "rb2_hip_multi_rank1a", "rb2_hip_multi_stats", "rb2_hip_multi_text_bytes",
]


_NT6 = np.full(256, 255, dtype=np.uint8)     # pattern letters: ACGTN in either case, '$' (a string end); anything else is refused
for _i, _ch in enumerate("$ACGTN"):
    _NT6[ord(_ch)] = _NT6[ord(_ch.lower())] = _i


def encode_pattern(p):
    """a pattern as nt6 codes in text order: str / bytes over $ACGTN (any case), or an array of codes (taken as they are)"""
    if isinstance(p, str):
        p = p.encode("ascii")
    if isinstance(p, (bytes, bytearray)):
        a = _NT6[np.frombuffer(bytes(p), dtype=np.uint8)]
        if (a == 255).any():
            raise ValueError("pattern %r: only the letters $ACGTN are allowed" % (p,))
        return a
    return np.asarray(p, dtype=np.uint8).reshape(-1)


def pack_patterns(patterns):
    """list of patterns -> (concatenated nt6 codes, offsets of n + 1 values): the layout of rb2_hip_backward_search"""
    enc = [encode_pattern(p) for p in patterns]
    off = np.zeros(len(enc) + 1, np.int64)
    if enc:
        off[1:] = np.cumsum([len(e) for e in enc])
    pat = np.concatenate(enc) if enc and off[-1] else np.zeros(1, np.uint8)
    return np.ascontiguousarray(pat, dtype=np.uint8), off


def pack_kmer(seq):
    """the code of a k-mer (str / bytes over ACGT, or nt6 codes 1..4; k = 1 .. 32) as rb2_hip_kmers reports it: two bits per symbol,
    A C G T = 0 1 2 3, the first symbol in the highest bits, so that codes of one k sort as the k-mers do"""
    a = encode_pattern(seq).astype(np.uint64)
    if not 1 <= len(a) <= 32 or (a < 1).any() or (a > 4).any():
        raise ValueError("k-mer %r: 1 .. 32 symbols out of ACGT" % (seq,))
    return np.uint64(((a - np.uint64(1)) << (np.uint64(2) * np.arange(len(a) - 1, -1, -1, dtype=np.uint64))).sum())


def unpack_kmers(codes, k):
    """codes of k-mers (rb2_hip_kmers) -> an (n, k) uint8 array of nt6 codes 1..4 in text order"""
    codes = np.asarray(codes, dtype=np.uint64).reshape(-1)
    sh = np.uint64(2) * np.arange(k - 1, -1, -1, dtype=np.uint64)
    return ((codes[:, None] >> sh[None, :]) & np.uint64(3)).astype(np.uint8) + np.uint8(1)


def pack_subs(subs):
    """substitutions [(pos, sym), ...] of a match (at most four, positions below 8192, nt6 codes 1..4) -> the subs word of rb2_hip_approx:
    16 bits each as pos << 3 | sym, in decreasing pos, the first in bits 0..15"""
    subs = sorted(((int(p), int(c)) for p, c in subs), reverse=True)
    if len(subs) > 4 or any(not (0 <= p < 8192 and 1 <= c <= 4) for p, c in subs) or len({p for p, _ in subs}) != len(subs):
        raise ValueError("substitutions %r: at most four (pos, sym) with distinct pos < 8192 and sym in 1..4" % (subs,))
    return sum((p << 3 | c) << (16 * k) for k, (p, c) in enumerate(subs))


def unpack_subs(subs):
    """the subs word of a record of rb2_hip_approx -> [(pos, sym), ...] in decreasing pos: text position, nt6 code the match has there"""
    subs = int(subs) & 0xFFFFFFFFFFFFFFFF
    out = []
    while subs & 0xFFFF:
        out.append(((subs & 0xFFFF) >> 3, subs & 7))
        subs >>= 16
    return out


class StepBudgetExceeded(RuntimeError):
    """HipBwt.approx, HipBwt.irreducible, HipBwt.correct: some queries used up max_steps before their search ended; .queries lists them, .results holds
    what the call would have returned, with what those queries had found so far"""
    def __init__(self, queries, results, who="approx", lower="max_mm", budget="max_steps"):
        RuntimeError.__init__(self, "%s: %d queries ran out of steps (the first: %s); raise %s or lower %s" % (who, len(queries), queries[:5], budget, lower))
        self.queries, self.results = queries, results


def budget_have(cnt, cap):
    """the records an item holds, from cnt as the searches with a step budget report it (>= 0 found, -1 malformed, <= -2 out of steps
    with -2 - cnt found by then): what it found, cap at the most"""
    return np.minimum(np.where(cnt <= -2, -2 - cnt, np.maximum(cnt, 0)), cap)


def raise_over_budget(cnt, results, *names):
    """StepBudgetExceeded(the items with cnt <= -2, results, *names) when there is such an item"""
    over = np.flatnonzero(cnt <= -2)
    if len(over):
        raise StepBudgetExceeded(over.tolist(), results, *names)


def expand_runs(rle):
    """1-byte-run 43+3 stream (what the device emits) -> nt6 symbols."""
    rle = np.asarray(rle, dtype=np.uint8)
    return np.repeat(rle & 7, rle >> 3)


def encode_runs(symbols):
    """nt6 symbols -> 43+3 stream using the 1/2/4/8-byte forms (rle.h:53-75); host-side helper."""
    symbols = np.asarray(symbols, dtype=np.uint8)
    out = bytearray()
    if len(symbols) == 0:
        return np.zeros(0, np.uint8)
    edges = np.flatnonzero(np.diff(symbols)) + 1
    starts = np.concatenate([[0], edges])
    lens = np.diff(np.concatenate([starts, [len(symbols)]]))
    for c, l in zip(symbols[starts].tolist(), lens.tolist()):
        if l < 16:
            out.append(l << 3 | c)
        else:
            n = 2 if l < 256 else 4 if l < (1 << 19) else 8
            tail = []
            for _ in range(n - 1):
                tail.append(0x80 | (l & 0x3f))
                l >>= 6
            out.append({2: 0xC0, 4: 0xE0, 8: 0xF0}[n] | l << 3 | c)
            out.extend(reversed(tail))
    return np.frombuffer(bytes(out), dtype=np.uint8)


def _fmd_image(src):
    """an .fmd as one contiguous uint8 array: the file behind a path, or bytes / a uint8 array as they are"""
    if isinstance(src, (str, os.PathLike)):
        return np.fromfile(os.fspath(src), dtype=np.uint8)
    if isinstance(src, (bytes, bytearray, memoryview)):
        return np.frombuffer(src, dtype=np.uint8)
    return np.ascontiguousarray(src, dtype=np.uint8).reshape(-1)


def _stored(cnt, cap, what):
    """how many of its records every item of a *_raw result holds, min(cnt, cap); an item with cnt < 0 raises ValueError: what, and
    the first five of them"""
    if (cnt < 0).any():
        raise ValueError("%s: %s" % (what, np.flatnonzero(cnt < 0)[:5].tolist()))
    return np.minimum(cnt, cap)


class HipBwt:
    """Six-rope BWT resident in the HBM of one MI355X."""

    def __init__(self, sorting_order=0, device=0):
        self.L = load_hip_lib()
        if self.L.rb2_hip_device_count() <= 0:
            raise RuntimeError("no HIP device visible: the gfx950 engine has no CPU fallback")
        self.h = self.L.rb2_hip_create(device, sorting_order)
        self.so = sorting_order
        self.dev = device

    def close(self):
        if getattr(self, "h", None):
            self.L.rb2_hip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        """empty index again; grown buffers are kept"""
        self.L.rb2_hip_reset(self.h)

    # -- the hot path ---------------------------------------------------------------------
    def insert_multi(self, buf):
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        self.L.rb2_hip_insert_multi(self.h, len(buf), buf.ctypes.data)

    def insert_multi_dev(self, dev_ptr, nbytes):
        self.L.rb2_hip_insert_multi_dev(self.h, nbytes, dev_ptr)

    def set_lazy(self, on):
        """rb2_hip_set_lazy: may insert_multi return before the device is done with the batch (default: yes)"""
        self.L.rb2_hip_set_lazy(self.h, int(on))

    def wait(self):
        self.L.rb2_hip_wait(self.h)

    def last_batch_counts(self):
        """what the last insert_multi adds to counts(), from the text of the batch alone (None if it was not a host-buffer insert)"""
        d = np.zeros(36, np.int64)
        return d.reshape(6, 6) if self.L.rb2_hip_last_batch_counts(self.h, d.ctypes.data) else None

    def prefetch(self, buf, n_final, capacity=0):
        """start uploading buf[:n_final] for a later insert_multi(buf[:len]) (rb2_hip_prefetch); buf must stay alive and in place"""
        self.L.rb2_hip_prefetch(self.h, buf.ctypes.data, n_final, capacity or len(buf))

    # -- state ----------------------------------------------------------------------------
    def counts(self):
        c = np.zeros(36, np.int64)
        self.L.rb2_hip_get_counts(self.h, c.ctypes.data)
        return c.reshape(6, 6)

    def rope_rle(self, b):
        n = self.L.rb2_hip_rope_bytes(self.h, b)
        out = np.zeros(max(n, 1), np.uint8)
        got = self.L.rb2_hip_download_rope(self.h, b, out.ctypes.data)
        assert got == n
        return out[:n]

    def rope(self, b):
        return expand_runs(self.rope_rle(b))

    def ropes(self):
        return [self.rope(b) for b in range(6)]

    def bwt(self):
        return np.concatenate(self.ropes())

    def load_ropes(self, rles):
        arrs = [np.ascontiguousarray(r, dtype=np.uint8) for r in rles]
        ptrs = (C.c_void_p * 6)(*[a.ctypes.data if len(a) else None for a in arrs])
        lens = (C.c_int64 * 6)(*[len(a) for a in arrs])
        self.L.rb2_hip_load_ropes(self.h, ptrs, lens)

    def load_fmd(self, src):
        """replace the index by the one an .fmd holds (rb2_hip_load_fmd); src: a path, or the file image as bytes / a uint8 array.
        Returns the number of symbols loaded.  The sorting order stays the one the handle was created with."""
        if isinstance(src, (str, os.PathLike)):
            return int(self.L.rb2_hip_load_fmd_file(self.h, os.fsencode(src)))
        img = _fmd_image(src)
        return int(self.L.rb2_hip_load_fmd(self.h, img.ctypes.data, len(img)))

    def save_fmd(self, path=None):
        """the index as an .fmd image (rb2_hip_save_fmd): what `ropebwt2 -d` writes for the same BWT, byte for byte.  Without a path the image
        comes back as a uint8 array; with one it is written there and its size is returned (OSError when the file cannot be written)."""
        if path is not None:
            n = int(self.L.rb2_hip_save_fmd_file(self.h, os.fsencode(path)))
            if n < 0:
                raise OSError("cannot write %s" % (path,))
            return n
        size = int(self.L.rb2_hip_save_fmd(self.h, None, 0))
        img = np.empty(size, dtype=np.uint8)
        got = int(self.L.rb2_hip_save_fmd(self.h, img.ctypes.data, size))
        assert got == size, (got, size)
        return img

    def delete(self, ids):
        """take the strings with these ids (rows of the $ block: what extract() takes and locate() gives; any integer sequence or
        array, in any order, duplicates allowed) out of the index (rb2_hip_delete_strings).  The index becomes the BWT of the
        remaining strings, whose ids close ranks; a sampled suffix array is dropped.  Returns the rows removed"""
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(-1))
        return int(self.L.rb2_hip_delete_strings(self.h, len(ids), ids.ctypes.data))

    def delete_stats(self):
        """what the last delete() met (rb2_hip_delete_stats)"""
        a = np.zeros(5, np.int64)
        self.L.rb2_hip_delete_stats(self.h, a.ctypes.data)
        return {"rows_removed": int(a[0]), "groups": int(a[1]), "groups_compressed": int(a[2]), "leaves_read": int(a[3]), "leaves_written": int(a[4])}

    def reserve(self, batch_bytes=0, batch_strings=0, total_symbols=0):
        self.L.rb2_hip_reserve(self.h, batch_bytes, batch_strings, total_symbols)

    def rope_hashes(self):
        """device-side checksums of the six ropes (rb2_hip_rope_hash)"""
        return [int(self.L.rb2_hip_rope_hash(self.h, b)) for b in range(6)]

    def rank1a(self, b, x):
        c = np.zeros(6, np.int64)
        self.L.rb2_hip_rank1a(self.h, b, x, c.ctypes.data)
        return c

    def rank_batch(self, b, xs):
        """counts of the six symbols in [0, x) of rope b for every x in xs (one launch, one wave per query)"""
        xs = np.ascontiguousarray(xs, dtype=np.int64)
        out = np.zeros((len(xs), 6), np.int64)
        if len(xs):
            self.L.rb2_hip_rank_batch(self.h, b, len(xs), xs.ctypes.data, out.ctypes.data)
        return out

    # -- FM-index queries (include/rb2_hip.h: global rows over ropes $ .. N, patterns in text order) ------------------------
    def backward_search(self, patterns):
        """lo, hi, m (int64 arrays): [lo, hi) is the interval of the longest suffix of each pattern that occurs, m its length;
        (0, N, 0) for the empty pattern, (-1, -1, -1) for a malformed one ('$' anywhere but at the end)"""
        pat, off = pack_patterns(patterns)
        n = len(off) - 1
        out = np.zeros((n, 3), np.int64)
        if n:
            self.L.rb2_hip_backward_search(self.h, n, pat.ctypes.data, off.ctypes.data, out.ctypes.data)
        return out[:, 0], out[:, 1], out[:, 2]

    def backward_search_dev(self, n, pat_dev, off_dev, out_dev):
        """rb2_hip_backward_search_dev: all three pointers in this device's memory; asynchronous on the handle's stream"""
        self.L.rb2_hip_backward_search_dev(self.h, n, pat_dev, off_dev, out_dev)

    def count(self, patterns):
        """occurrences of every pattern (str / bytes over $ACGTN, or nt6 arrays) in the indexed strings"""
        lens = np.array([len(encode_pattern(p)) for p in patterns], np.int64)
        lo, hi, m = self.backward_search(patterns)
        return np.where(m == lens, hi - lo, 0)

    def extend(self, ik, is_back):
        """rld_extend on bi-intervals ik (n, 3) = x[0], x[1], x[2]: an (n, 6, 3) array, [i, a] = the extension of ik[i] by a"""
        ik = np.ascontiguousarray(np.asarray(ik, dtype=np.int64).reshape(-1, 3))
        ok = np.zeros((len(ik), 6, 3), np.int64)
        if len(ik):
            self.L.rb2_hip_extend(self.h, len(ik), ik.ctypes.data, int(bool(is_back)), ok.ctypes.data)
        return ok

    def extract(self, rows, max_len):
        """the strings of rows of the $ block, in text order (one nt6 array per row); None where the string is longer than
        max_len; a row outside the $ block raises ValueError"""
        rows = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1))
        n = len(rows)
        out = np.zeros(max(n * max_len, 1), np.uint8)
        ln = np.zeros(n, np.int64)
        if n:
            self.L.rb2_hip_extract(self.h, n, rows.ctypes.data, max_len, out.ctypes.data, ln.ctypes.data)
        if (ln == -2).any():
            raise ValueError("rows outside the $ block: %s" % rows[ln == -2][:5].tolist())
        return [out[i * max_len:i * max_len + ln[i]].copy() if ln[i] >= 0 else None for i in range(n)]

    def extract_raw(self, rows, max_len):
        """rb2_hip_extract as it is: (number of rows that fitted, out (n, max_len) uint8, len (n,) int64)"""
        rows = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1))
        out = np.zeros((len(rows), max_len), np.uint8)
        ln = np.zeros(len(rows), np.int64)
        fit = self.L.rb2_hip_extract(self.h, len(rows), rows.ctypes.data, max_len, out.ctypes.data, ln.ctypes.data) if len(rows) else 0
        return int(fit), out, ln

    def _records(self, fn, n, args, cap, words, call_empty):
        """(records stored, rec (n, cap, words) int64, cnt (n,) int64) of fn(h, n, *args, rec, cnt), one of the host variants that return
        records; rec and cnt start as zeros, and without items fn is called only if call_empty (its checks still run then)"""
        rec = np.zeros((n, max(int(cap), 0), words), np.int64)
        cnt = np.zeros(n, np.int64)
        stored = fn(self.h, n, *args, rec.ctypes.data, cnt.ctypes.data) if n or call_empty else 0
        return int(stored), rec, cnt

    def smem_raw(self, queries, min_len=1, min_occ=1, max_mems=64):
        """rb2_hip_smem as it is: (records stored, mem (n, max_mems, 5) int64 = start, end, x0, x1, size, cnt (n,) int64); only the
        first min(cnt[i], max_mems) records of query i are meaningful (the others are zeros), cnt[i] = -1 for a malformed query"""
        qry, off = pack_patterns(queries)
        return self._records(self.L.rb2_hip_smem, len(off) - 1, (qry.ctypes.data, off.ctypes.data, min_len, min_occ, max_mems), max_mems, 5, False)

    def smem(self, queries, min_len=1, min_occ=1, max_mems=64):
        """super-maximal exact matches of every query (str / bytes over ACGTN, or nt6 arrays) against an index that holds both strands:
        a list with one (k, 5) int64 array per query, rows = start, end, x0, x1, size in increasing start, k = min(cnt, max_mems), and
        cnt (n,) = the SMEMs found per query; a malformed query ('$' or a code above 5 inside) raises ValueError"""
        stored, mem, cnt = self.smem_raw(queries, min_len, min_occ, max_mems)
        return [m[:k].copy() for m, k in zip(mem, _stored(cnt, max_mems, "malformed queries (only the codes 1..5 are allowed)"))], cnt

    def smem_dev(self, n, qry_dev, off_dev, mem_dev, cnt_dev, min_len=1, min_occ=1, max_mems=64):
        """rb2_hip_smem_dev: all four pointers in this device's memory; asynchronous on the handle's stream"""
        self.L.rb2_hip_smem_dev(self.h, n, qry_dev, off_dev, min_len, min_occ, max_mems, mem_dev, cnt_dev)

    # -- sampled suffix array: rows back to (string id, position) (include/rb2_hip.h) ----------------------------------------
    def build_ssa(self, log2_step=5):
        """rb2_hip_ssa_build: sample every row that is a multiple of 2**log2_step; returns the samples stored.  Valid until the
        index changes (an insert, a load, reset)"""
        return int(self.L.rb2_hip_ssa_build(self.h, int(log2_step)))

    def drop_ssa(self):
        self.L.rb2_hip_ssa_drop(self.h)

    def ssa_info(self):
        a = np.zeros(4, np.int64)
        self.L.rb2_hip_ssa_info(self.h, a.ctypes.data)
        return {"valid": bool(a[0]), "log2_step": int(a[1]), "samples": int(a[2]), "device_bytes": int(a[3])}

    def locate_raw(self, intervals, max_hits):
        """rb2_hip_locate as it is: (records stored, hit (n, max_hits, 2) int64 = string id, position, cnt (n,) int64); only the first
        min(cnt[i], max_hits) records of interval i are meaningful (the others are zeros), cnt[i] = -1 for a malformed interval"""
        iv = np.ascontiguousarray(np.asarray(intervals, dtype=np.int64).reshape(-1, 2))
        return self._records(self.L.rb2_hip_locate, len(iv), (iv.ctypes.data, max_hits), max_hits, 2, True)

    def locate(self, intervals, max_hits=64):
        """the places of the rows of every interval (lo, hi): a list with one (m, 2) int64 array per interval, rows = string id,
        position (0-based, text order) in row order, m = min(hi - lo, max_hits); a malformed interval raises ValueError"""
        stored, hit, cnt = self.locate_raw(intervals, max_hits)
        return [m[:k].copy() for m, k in zip(hit, _stored(cnt, max_hits, "malformed intervals (0 <= lo <= hi <= rows)"))]

    def locate_dev(self, n, iv_dev, hit_dev, cnt_dev, max_hits=64):
        """rb2_hip_locate_dev: all three pointers in this device's memory; asynchronous on the handle's stream"""
        self.L.rb2_hip_locate_dev(self.h, n, iv_dev, max_hits, hit_dev, cnt_dev)

    def find(self, patterns, max_hits=64):
        """where every pattern (str / bytes over $ACGTN, or nt6 arrays) occurs: backward search, then locate for the patterns that
        matched in full.  One (m, 2) int64 array per pattern, rows = string id, position of the pattern's first symbol, at most
        max_hits of them; empty for a pattern that does not occur"""
        lens = np.array([len(encode_pattern(p)) for p in patterns], np.int64)
        lo, hi, m = self.backward_search(patterns)
        full = np.flatnonzero(m == lens)
        out = [np.zeros((0, 2), np.int64) for _ in patterns]
        if len(full):
            for i, h in zip(full, self.locate(np.stack([lo[full], hi[full]], 1), max_hits)):
                out[i] = h
        return out

    # -- suffix-prefix overlaps: the strings that begin with a suffix of a query (include/rb2_hip.h) -------------------------
    def overlap_raw(self, queries, min_ovlp, max_recs):
        """rb2_hip_overlap as it is: (records stored, rec (n, max_recs, 3) int64 = length, zlo, zhi, cnt (n,) int64); only the first
        min(cnt[i], max_recs) records of query i are meaningful (the others are zeros), cnt[i] = -1 for a malformed query"""
        qry, off = pack_patterns(queries)
        return self._records(self.L.rb2_hip_overlap, len(off) - 1, (qry.ctypes.data, off.ctypes.data, min_ovlp, max_recs), max_recs, 3, False)

    def overlap_dev(self, n, qry_dev, off_dev, rec_dev, cnt_dev, min_ovlp, max_recs):
        """rb2_hip_overlap_dev: all four pointers in this device's memory; asynchronous on the handle's stream"""
        self.L.rb2_hip_overlap_dev(self.h, n, qry_dev, off_dev, min_ovlp, max_recs, rec_dev, cnt_dev)

    def string_ids_raw(self, ranges, max_hits):
        """rb2_hip_string_ids as it is: (ids stored, ids (n, max_hits) int64, cnt (n,) int64); only the first min(cnt[i], max_hits) ids
        of range i are meaningful (the others are zeros), cnt[i] = -1 for a malformed range.  Needs build_ssa()"""
        zv = np.ascontiguousarray(np.asarray(ranges, dtype=np.int64).reshape(-1, 2))
        stored, ids, cnt = self._records(self.L.rb2_hip_string_ids, len(zv), (zv.ctypes.data, max_hits), max_hits, 1, True)
        return stored, ids[:, :, 0], cnt

    def string_ids_dev(self, n, zv_dev, ids_dev, cnt_dev, max_hits=64):
        """rb2_hip_string_ids_dev: all three pointers in this device's memory; asynchronous on the handle's stream"""
        self.L.rb2_hip_string_ids_dev(self.h, n, zv_dev, max_hits, ids_dev, cnt_dev)

    def overlaps(self, queries, min_ovlp, max_hits=64):
        """the strings of the index that begin with a suffix of at least min_ovlp symbols of each query (str / bytes over ACGTN, or nt6
        arrays): per query the list of (string id, overlap length), longest overlap first, at most max_hits strings per length.  The
        whole query counts as a suffix of itself, so a query that is in the index finds itself, its copies and the strings it is a proper
        prefix of.  Needs build_ssa() (none is built here); a malformed query ('$' or a code above 5 inside) raises ValueError"""
        lens = [len(encode_pattern(q)) for q in queries]
        max_recs = max(max(lens, default=0) - int(min_ovlp) + 1, 1)                  # one record per length at the most: nothing is cut
        _, rec, cnt = self.overlap_raw(queries, min_ovlp, max_recs)
        live = np.arange(max_recs)[None, :] < _stored(cnt, max_recs, "malformed queries (only the codes 1..5 are allowed)")[:, None]
        who = np.nonzero(live)[0]
        recs = rec[live]
        max_hits = max(min(int(max_hits), int((recs[:, 2] - recs[:, 1]).max(initial=1))), 1)    # no wider than the widest range
        _, ids, n_ids = self.string_ids_raw(recs[:, 1:], max_hits)
        out = [[] for _ in queries]
        for i, l, k, row in zip(who.tolist(), recs[:, 0].tolist(), np.minimum(n_ids, max_hits).tolist(), ids.tolist()):
            out[i].append([(s, l) for s in row[:k]])
        return [[p for grp in reversed(o) for p in grp] for o in out]

    # -- k-mer enumeration: the k-mers of the indexed strings and their counts (include/rb2_hip.h) ------------------------------
    def kmers_raw(self, k, min_occ=1, canonical=False, max_recs=1 << 16, hist_len=0):
        """rb2_hip_kmers as it is: (k-mers found, rec (max_recs, 3) int64 = code, lo, hi, hist (hist_len,) int64, info (4,) int64); only
        the first min(found, max_recs) records are meaningful (the others are zeros), in no particular order"""
        rec = np.zeros((max(int(max_recs), 0), 3), np.int64)
        hist = np.zeros(max(int(hist_len), 0), np.int64)
        info = np.zeros(4, np.int64)
        found = self.L.rb2_hip_kmers(self.h, int(k), int(min_occ), int(bool(canonical)), int(max_recs), rec.ctypes.data if len(rec) else None,
                                     int(hist_len), hist.ctypes.data if len(hist) else None, info.ctypes.data)
        return int(found), rec, hist, info

    def kmers(self, k, min_occ=1, canonical=False):
        """every distinct k-mer of the indexed strings with at least min_occ occurrences: (codes uint64, lo, hi), sorted by lo, which
        is the order of the codes and of the k-mers; hi - lo = occurrences, [lo, hi) goes to locate() as it is.  canonical: only the
        smaller of a k-mer and its reverse complement (an index of both strands).  One call when the k-mers fit the first guess, else one
        to count and one to fetch"""
        found, rec, _, _ = self.kmers_raw(k, min_occ, canonical)
        if found > len(rec):
            found, rec, _, _ = self.kmers_raw(k, min_occ, canonical, max_recs=found)
        rec = rec[:found]
        rec = rec[np.argsort(rec[:, 1], kind="stable")]
        return rec[:, 0].astype(np.uint64), rec[:, 1].copy(), rec[:, 2].copy()

    def kmer_spectrum(self, k, hist_len=256, min_occ=1, canonical=False):
        """the k-mer spectrum: hist[c] = distinct k-mers with exactly c occurrences, hist[hist_len - 1] = those with that many or more
        (no records are fetched)"""
        return self.kmers_raw(k, min_occ, canonical, max_recs=0, hist_len=hist_len)[2]

    # -- approximate search: the matches of a query within max_mm substitutions (include/rb2_hip.h) ---------------------------------
    def approx_raw(self, queries, max_mm, min_occ=1, max_steps=1 << 16, max_recs=64):
        """rb2_hip_approx as it is: (records stored, rec (n, max_recs, 4) int64 = lo, hi, n_mm, subs, cnt (n,) int64).  cnt[i] >= 0: the
        matches found, min(cnt[i], max_recs) of them stored; -1: a malformed query; <= -2: the query ran out of steps with -2 - cnt[i]
        matches found, min(that, max_recs) stored.  The records not stored are zeros, the order of a query's records is unspecified"""
        qry, off = pack_patterns(queries)
        return self._records(self.L.rb2_hip_approx, len(off) - 1, (qry.ctypes.data, off.ctypes.data, int(max_mm), min_occ, max_steps, max_recs), max_recs, 4, False)

    def approx(self, queries, max_mm, min_occ=1, max_steps=1 << 16, max_recs=64):
        """the words within max_mm substitutions of every query (str / bytes over ACGTN, or nt6 arrays) that occur at least min_occ times:
        per query a list of (lo, hi, n_mm, [(pos, sym), ...]) sorted by lo -- [lo, hi) goes to locate() as it is, the match has the nt6 code
        sym at text position pos and the query's symbols elsewhere --, at most max_recs of them, or None for a malformed query ('$' or a code
        above 5 inside, more than 8192 symbols).  Raises StepBudgetExceeded when a query used up max_steps: the exception names the queries
        and carries the results, partial for those"""
        _, rec, cnt = self.approx_raw(queries, max_mm, min_occ, max_steps, max_recs)
        have = budget_have(cnt, max_recs)
        out = [None if c == -1 else sorted((int(lo), int(hi), int(mm), unpack_subs(sb)) for lo, hi, mm, sb in r[:k].tolist()) for r, k, c in zip(rec, have, cnt)]
        raise_over_budget(cnt, out)
        return out

    def approx_dev(self, n, qry_dev, off_dev, rec_dev, cnt_dev, max_mm, min_occ=1, max_steps=1 << 16, max_recs=64):
        """rb2_hip_approx_dev: all four pointers in this device's memory; asynchronous on the handle's stream"""
        self.L.rb2_hip_approx_dev(self.h, n, qry_dev, off_dev, int(max_mm), min_occ, max_steps, max_recs, rec_dev, cnt_dev)

    # -- approximate search with insertions and deletions: the matches of a query within max_ed edits (include/rb2_hip.h) -----------
    def approx_ed_raw(self, queries, max_ed, min_occ=1, max_steps=1 << 16, max_recs=64):
        """rb2_hip_approx_ed as it is: (records stored, rec (n, max_recs, 4) int64 = lo, hi, ed, len, cnt (n,) int64).  cnt[i] >= 0: the
        matches found, min(cnt[i], max_recs) of them stored; -1: a malformed query; <= -2: the query ran out of steps with -2 - cnt[i]
        matches found, min(that, max_recs) stored.  The records not stored are zeros, the order of a query's records is unspecified"""
        qry, off = pack_patterns(queries)
        return self._records(self.L.rb2_hip_approx_ed, len(off) - 1, (qry.ctypes.data, off.ctypes.data, int(max_ed), min_occ, max_steps, max_recs), max_recs, 4, False)

    def approx_ed(self, queries, max_ed, min_occ=1, max_steps=1 << 16, max_recs=64):
        """the words within max_ed edits (substitutions, insertions, deletions; the first and last symbols aligned to those of the query) of
        every query (str / bytes over ACGTN, or nt6 arrays) that occur at least min_occ times: per query a sorted list of (lo, hi, ed, len)
        -- [lo, hi) goes to locate() as it is, the match has len symbols and the edit distance ed to the query --, at most max_recs of them,
        or None for a malformed query ('$' or a code above 5 inside, more than 8192 symbols).  Raises StepBudgetExceeded when a query used up
        max_steps: the exception names the queries and carries the results, partial for those"""
        _, rec, cnt = self.approx_ed_raw(queries, max_ed, min_occ, max_steps, max_recs)
        have = budget_have(cnt, max_recs)
        out = [None if c == -1 else sorted(map(tuple, r[:k].tolist())) for r, k, c in zip(rec, have, cnt)]
        raise_over_budget(cnt, out, "approx_ed", "max_ed")
        return out

    def approx_ed_dev(self, n, qry_dev, off_dev, rec_dev, cnt_dev, max_ed, min_occ=1, max_steps=1 << 16, max_recs=64):
        """rb2_hip_approx_ed_dev: all four pointers in this device's memory; asynchronous on the handle's stream"""
        self.L.rb2_hip_approx_ed_dev(self.h, n, qry_dev, off_dev, int(max_ed), min_occ, max_steps, max_recs, rec_dev, cnt_dev)

    # -- duplicate and contained strings (include/rb2_hip.h) -------------------------------------------------------------------------
    def contained_raw(self, ids=None):
        """rb2_hip_contained as it is: an (n, 5) int64 array, rows = flag, occ, n_equal, rank, walked of the strings ids (any integer
        sequence or array; None: every string of the index).  flag: bit 0 a copy of a string before it, bit 1 inside another string,
        4 an empty string, -1 an id that is no string, -2 a walk that did not end"""
        if ids is None:
            n, p = int(self.counts()[:, 0].sum()), None
        else:
            ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(-1))
            n, p = len(ids), ids.ctypes.data
        rec = np.zeros((n, 5), np.int64)
        if n:
            self.L.rb2_hip_contained(self.h, n, p, rec.ctypes.data)
        return rec

    def contained_dev(self, n, ids_dev, rec_dev):
        """rb2_hip_contained_dev: ids_dev (None or 0: the ids 0 .. n-1) and rec_dev (5 n int64) in this device's memory; asynchronous on
        the handle's stream"""
        self.L.rb2_hip_contained_dev(self.h, n, ids_dev or None, rec_dev)

    def contained(self, ids=None):
        """the flags of contained_raw alone: 0 for a string that is the first of its text and lies inside no other"""
        return self.contained_raw(ids)[:, 0].copy()

    def reduce(self, duplicates=True, contained=True, empty=True, pairs=False):
        """delete the copies (flag bit 0), the strings that lie inside another (bit 1) and the empty strings, as chosen, and return their
        old ids, sorted: contained_raw() followed by delete().  pairs: the index holds both strands, strings 2i and 2i+1 a read and its
        reverse complement, and a pair goes only when both its members are selected (a palindromic read and its copy stay together);
        an odd number of strings raises ValueError"""
        flag = self.contained_raw()[:, 0]
        sel = np.zeros(len(flag), bool)
        live = (flag >= 1) & (flag <= 3)
        if duplicates:
            sel |= live & ((flag & 1) != 0)
        if contained:
            sel |= live & ((flag & 2) != 0)
        if empty:
            sel |= flag == 4
        if pairs:
            if len(flag) % 2:
                raise ValueError("reduce(pairs=True): %d strings are no pairs of strands" % len(flag))
            sel = np.repeat(sel[0::2] & sel[1::2], 2)
        ids = np.flatnonzero(sel).astype(np.int64)
        if len(ids):
            self.delete(ids)
        return ids

    # -- irreducible overlaps: the edges of a string graph (include/rb2_hip.h) -----------------------------------------------------
    def irreducible_raw(self, queries, min_ovlp, max_ext, max_steps=1 << 16, max_recs=16):
        """rb2_hip_irreducible as it is: (records stored, rec (n, max_recs, 4) int64 = l, ext, zlo, zhi, cnt (n,) int64).  [zlo, zhi) are
        `$` ranks for string_ids_raw and name the REVERSE COMPLEMENTS of the neighbours.  cnt[i] >= 0: the records found, min(cnt[i],
        max_recs) of them stored; -1: a malformed query; <= -2: out of steps with -2 - cnt[i] records found.  The records not stored are
        zeros, the order of a query's records is unspecified"""
        qry, off = pack_patterns(queries)
        return self._records(self.L.rb2_hip_irreducible, len(off) - 1, (qry.ctypes.data, off.ctypes.data, min_ovlp, max_ext, max_steps, max_recs), max_recs, 4, False)

    def irreducible_dev(self, n, qry_dev, off_dev, rec_dev, cnt_dev, max_len, min_ovlp, max_ext, max_steps=1 << 16, max_recs=16):
        """rb2_hip_irreducible_dev: all four pointers in this device's memory; asynchronous on the handle's stream.  A query of more than
        max_len (1 .. 8192) symbols is malformed"""
        self.L.rb2_hip_irreducible_dev(self.h, n, qry_dev, off_dev, max_len, min_ovlp, max_ext, max_steps, max_recs, rec_dev, cnt_dev)

    def irreducible(self, queries, min_ovlp, max_ext=None, max_steps=1 << 16, max_recs=16, max_hits=8, pairs=False):
        """the irreducible overlaps of every query (str / bytes over ACGTN, or nt6 arrays) with the strings of an index of both strands:
        per query the sorted list of (string id, l, ext) -- the string continues the query by ext symbols behind an overlap of l, and no
        other such string lies on the way to it --, at most max_recs distinct (l, extension) per query and max_hits strings of each; None
        for a malformed query.  The ids are those of the REVERSE COMPLEMENTS of the neighbours (that is what the index yields) unless
        pairs: then the index is taken to hold a read and its reverse complement as the strings 2i and 2i + 1 (input order, as
        reduce(pairs=True) leaves it) and the id returned is id ^ 1, the neighbour itself; ValueError for another sorting order or an
        odd number of strings.  max_ext=None: the longest query.  Needs build_ssa() (none is built here).  Raises StepBudgetExceeded
        as approx() does"""
        if pairs and (self.so != 0 or int(self.counts()[:, 0].sum()) % 2):
            raise ValueError("irreducible(pairs=True): the index must be in input order and hold an even number of strings")
        if max_ext is None:
            max_ext = min(max(max((len(encode_pattern(q)) for q in queries), default=1), 1), 8192)
        _, rec, cnt = self.irreducible_raw(queries, min_ovlp, max_ext, max_steps, max_recs)
        have = budget_have(cnt, max_recs)
        live = np.arange(max_recs)[None, :] < have[:, None]
        who = np.nonzero(live)[0]
        recs = rec[live]
        out = [None if c == -1 else [] for c in cnt.tolist()]
        if len(recs):
            max_hits = max(min(int(max_hits), int((recs[:, 3] - recs[:, 2]).max())), 1)          # no wider than the widest range
            _, ids, n_ids = self.string_ids_raw(recs[:, 2:], max_hits)
            for i, l, e, k, row in zip(who.tolist(), recs[:, 0].tolist(), recs[:, 1].tolist(), np.minimum(n_ids, max_hits).tolist(), ids.tolist()):
                out[i] += [(s ^ 1 if pairs else s, l, e) for s in row[:k]]
        out = [o if o is None else sorted(o) for o in out]
        raise_over_budget(cnt, out, "irreducible", "max_ext")
        return out

    def edges(self, ids=None, min_ovlp=1, **kw):
        """the edges of the string graph that leave the strings ids (None: every string): their text is read with extract() and asked
        with irreducible(..., **kw).  An (m, 4) int64 array, rows = src, dst, l, ext sorted; dst as irreducible() names it (the neighbour
        itself with pairs=True)"""
        n = int(self.counts()[:, 0].sum())
        ids = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64).reshape(-1)
        if len(ids) == 0:
            return np.zeros((0, 4), np.int64)
        max_len = 64
        texts = self.extract(ids, max_len)
        while any(t is None for t in texts):                        # (longer than the guess: read again with room)
            max_len *= 4
            texts = self.extract(ids, max_len)
        res = self.irreducible(texts, min_ovlp, **kw)
        rows = [(int(s), d, l, e) for s, r in zip(ids.tolist(), res) for d, l, e in (r or [])]
        return np.array(sorted(rows), np.int64).reshape(-1, 4)

    # -- unitigs: the chains of a string graph and their texts (include/rb2_hip.h) ---------------------------------------------------
    def unitig_chains(self, edges, n_str=None):
        """rb2_hip_unitig_chains: the chains of the edge list edges (m, 4) int64 = src, dst, l, ext (what edges() returns) over n_str
        vertices (None: the strings of the index).  Returns (vtx (n_str, 4) int64 = head, rank, off, ext_in, info (4,) int64 = chains,
        cycles, vertices of the longest chain, edges ignored)"""
        edges = np.ascontiguousarray(np.asarray(edges, dtype=np.int64).reshape(-1, 4))
        n = int(self.counts()[:, 0].sum()) if n_str is None else int(n_str)
        vtx = np.zeros((max(n, 0), 4), np.int64)
        info = np.zeros(4, np.int64)
        self.L.rb2_hip_unitig_chains(self.h, n, len(edges), edges.ctypes.data, vtx.ctypes.data, info.ctypes.data)
        return vtx, info

    def unitig_chains_dev(self, n_str, m, edges_dev, vtx_dev, info_dev):
        """rb2_hip_unitig_chains_dev: all three pointers in this device's memory; asynchronous on the handle's stream"""
        self.L.rb2_hip_unitig_chains_dev(self.h, n_str, m, edges_dev, vtx_dev, info_dev)

    def unitig_text_raw(self, vtx, canonical=False, min_reads=1, cap_u=0, cap_txt=0, fill=0):
        """rb2_hip_unitig_text as it is: (chains stored, urec (cap_u, 5) int64, txt (cap_txt,) uint8, info (4,) int64 = chains selected,
        their total text length, those with a short piece, chains stored); urec and txt start as fill, and what belongs to a chain that
        is not stored stays so"""
        vtx = np.ascontiguousarray(np.asarray(vtx, dtype=np.int64).reshape(-1, 4))
        urec = np.full((max(int(cap_u), 0), 5), fill, np.int64)
        txt = np.full(max(int(cap_txt), 0), fill, np.uint8)
        info = np.zeros(4, np.int64)
        stored = self.L.rb2_hip_unitig_text(self.h, len(vtx), vtx.ctypes.data, int(bool(canonical)), int(min_reads), int(cap_u), int(cap_txt),
                                            urec.ctypes.data if len(urec) else None, txt.ctypes.data if len(txt) else None, info.ctypes.data)
        return int(stored), urec, txt, info

    def unitig_text(self, vtx, canonical=False, min_reads=1):
        """the texts of the chains vtx (unitig_chains) describes: one call with caps 0 for the sizes, one that stores.  Returns (urec (k, 5)
        int64 = head, n_reads, text_off, text_len, flags (bit 0 circular, bit 1 a short piece) of the selected chains by increasing head,
        txt uint8: the nt6 text of chain u is txt[text_off : text_off + text_len])"""
        _, _, _, info = self.unitig_text_raw(vtx, canonical, min_reads)
        stored, urec, txt, info = self.unitig_text_raw(vtx, canonical, min_reads, int(info[0]), int(info[1]))
        assert stored == len(urec) == info[0]
        return urec, txt

    def unitig_text_dev(self, n_str, vtx_dev, urec_dev, txt_dev, canonical=False, min_reads=1, cap_u=0, cap_txt=0):
        """rb2_hip_unitig_text_dev: vtx, urec (5 cap_u int64) and txt (cap_txt bytes) in this device's memory.  Synchronises the handle's
        stream once; returns (chains stored, info (4,) int64)"""
        info = np.zeros(4, np.int64)
        stored = self.L.rb2_hip_unitig_text_dev(self.h, n_str, vtx_dev, int(bool(canonical)), int(min_reads), int(cap_u), int(cap_txt), urec_dev or None, txt_dev or None,
                                                info.ctypes.data)
        return int(stored), info

    def unitigs(self, min_ovlp, canonical=True, min_reads=1, **kw):
        """the unitigs of the string graph of an index of both strands in input order, strings 2i and 2i + 1 a read and its reverse
        complement (as reduce(pairs=True) leaves it): edges(min_ovlp=min_ovlp, pairs=True, **kw), unitig_chains, unitig_text.  A list of
        (text as an nt6 uint8 array, the read ids in chain order, circular) by increasing head id; canonical: one of every unitig and
        its reverse complement.  Needs build_ssa() (none is built here)"""
        vtx, _ = self.unitig_chains(self.edges(min_ovlp=min_ovlp, pairs=True, **kw))
        urec, txt = self.unitig_text(vtx, canonical, min_reads)
        order = np.lexsort((vtx[:, 1], vtx[:, 0]))                  # by head, then by rank
        first = np.searchsorted(vtx[order, 0], urec[:, 0])
        return [(txt[o:o + l].copy(), order[f:f + k].copy(), bool(fl & 1)) for (hd, k, o, l, fl), f in zip(urec.tolist(), first.tolist())]

    # -- the string graph of the index's own strings, on the device (include/rb2_hip.h) ---------------------
    def _graph_args(self, who, first, n, max_ext, pairs):
        """(first, n, max_ext) with the defaults filled in: n = None: up to the last string; max_ext = None: the longest string of the
        index, read from the offsets of one sizing call (8 bytes a string: pass max_ext on an index where that matters)"""
        total = self._n_strings()
        if pairs and (self.so != 0 or total % 2):
            raise ValueError("%s(pairs=True): the index must be in input order and hold an even number of strings" % who)
        if n is None:
            n = total - first
        if max_ext is None:
            off = np.zeros(total + 1, np.int64)
            self.L.rb2_hip_unpack(self.h, 0, total, 0, 0, None, off.ctypes.data)
            max_ext = min(max(int(np.diff(off).max()) - 1 if total else 1, 1), 8192)
        return int(first), int(n), int(max_ext)

    def string_graph_dev(self, first, n, edges_dev, cap, min_ovlp=1, max_ext=8192, max_steps=1 << 16, max_recs=16, max_hits=8, pairs=False):
        """rb2_hip_string_graph_dev: edges_dev (4 cap int64; None or 0 with cap 0 counts only) in this device's memory.  Returns (m, info (8,)
        int64 = m, rows stored, sources over max_recs, records over max_hits, sources out of steps, sources over 8192 symbols, 0, 0)"""
        info = np.zeros(8, np.int64)
        m = self.L.rb2_hip_string_graph_dev(self.h, first, n, min_ovlp, max_ext, max_steps, max_recs, max_hits, int(bool(pairs)), int(cap), edges_dev or None, info.ctypes.data)
        return int(m), info

    def string_graph_raw(self, first, n, cap, min_ovlp=1, max_ext=8192, max_steps=1 << 16, max_recs=16, max_hits=8, pairs=False, fill=0):
        """rb2_hip_string_graph as it is: (m, edges (cap, 4) int64 that start as fill, info (8,) int64); cap 0 passes NULL"""
        edges = np.full((max(int(cap), 0), 4), fill, np.int64)
        info = np.zeros(8, np.int64)
        m = self.L.rb2_hip_string_graph(self.h, first, n, min_ovlp, max_ext, max_steps, max_recs, max_hits, int(bool(pairs)), int(cap), edges.ctypes.data if len(edges) else None,
                                        info.ctypes.data)
        return int(m), edges, info

    def string_graph(self, first=0, n=None, min_ovlp=1, max_ext=None, max_steps=1 << 16, max_recs=16, max_hits=8, pairs=False):
        """the edges of the string graph that leave the strings first .. first + n - 1 (n = None: up to the last), found on the device by
        one call: (edges (m, 4) int64 = src, dst, l, ext by increasing src, info (8,) int64 as string_graph_dev returns it).  dst as
        irreducible() names it: the reverse complement of the neighbour, or the neighbour itself with pairs=True (ValueError as there).
        Sizes with a guess of two edges a source and repeats once with cap = m when the guess was short.  A source that is cut by
        max_recs, max_hits or max_steps shows in info[2:5] only.  Needs build_ssa() (none is built here)"""
        first, n, max_ext = self._graph_args("string_graph", first, n, max_ext, pairs)
        kw = dict(min_ovlp=min_ovlp, max_ext=max_ext, max_steps=max_steps, max_recs=max_recs, max_hits=max_hits, pairs=pairs)
        m, edges, info = self.string_graph_raw(first, n, 2 * n + 16, **kw)
        if m > len(edges):
            m, edges, info = self.string_graph_raw(first, n, m, **kw)
        return edges[:m].copy(), info

    # -- tip and bubble removal on an edge list (include/rb2_hip.h) ------------------------------------------
    def graph_clean_dev(self, n_str, m, edges_dev, out_dev, cap, max_tip_reads=2, max_bubble_reads=3, pairs=True, max_rounds=8):
        """rb2_hip_graph_clean_dev: edges_dev (4 m int64) and out_dev (4 cap int64; None or 0 with cap 0 counts only) in this device's
        memory.  Returns (m', info (8,) int64 = m', rows stored, rounds, tip rows, bubble rows, rows ignored, chains of the result, 0)"""
        info = np.zeros(8, np.int64)
        kept = self.L.rb2_hip_graph_clean_dev(self.h, int(n_str), int(m), edges_dev or None, int(max_tip_reads), int(max_bubble_reads), int(bool(pairs)), int(max_rounds), int(cap),
                                              out_dev or None, info.ctypes.data)
        return int(kept), info

    def graph_clean_raw(self, edges, n_str, max_tip_reads, max_bubble_reads, pairs, max_rounds, cap, fill=0):
        """rb2_hip_graph_clean as it is: (m', out (cap, 4) int64 that starts as fill, info (8,) int64); no rows pass NULL, and so does cap 0"""
        edges = np.ascontiguousarray(np.asarray(edges, dtype=np.int64).reshape(-1, 4))
        out = np.full((max(int(cap), 0), 4), fill, np.int64)
        info = np.zeros(8, np.int64)
        kept = self.L.rb2_hip_graph_clean(self.h, int(n_str), len(edges), edges.ctypes.data if len(edges) else None, int(max_tip_reads), int(max_bubble_reads), int(pairs),
                                          int(max_rounds), int(cap), out.ctypes.data if len(out) else None, info.ctypes.data)
        return int(kept), out, info

    def graph_clean(self, edges, n_str=None, max_tip_reads=2, max_bubble_reads=3, pairs=True, max_rounds=8):
        """the edge list edges (m, 4) int64 = src, dst, l, ext over n_str vertices (None: the strings of the index) without its tips of at
        most max_tip_reads reads and the losing arms of its bubbles of at most max_bubble_reads reads (the rules: include/rb2_hip.h):
        (the rows kept, in input order, info (8,) int64 as graph_clean_dev returns it).  pairs: vertices 2i and 2i + 1 are one read"""
        edges = np.asarray(edges, dtype=np.int64).reshape(-1, 4)
        n = self._n_strings() if n_str is None else int(n_str)
        kept, out, info = self.graph_clean_raw(edges, n, max_tip_reads, max_bubble_reads, int(bool(pairs)), max_rounds, len(edges))
        return out[:kept].copy(), info

    def assemble(self, min_ovlp, canonical=True, min_reads=1, clean=None, **kw):
        """what unitigs() returns, with the graph, the chains and the texts made on the device: string_graph_dev, unitig_chains_dev and
        unitig_text_dev on buffers from dev_alloc; only the unitigs' records, their text and the chain order come back.  kw: max_ext,
        max_steps, max_recs, max_hits of string_graph().  Returns (unitigs, info): info = what string_graph_dev reports (info[2:6] != 0:
        sources whose edges were cut short, which unitigs() raises for or passes over in silence).
        clean: None, or a dict of max_tip_reads, max_bubble_reads, pairs, max_rounds (those left out: graph_clean_dev's defaults): the
        edge list goes through graph_clean_dev into a second buffer before the chains are made, and info is then the pair (what
        string_graph_dev reports, what graph_clean_dev reports)"""
        _, n, max_ext = self._graph_args("assemble", 0, None, kw.pop("max_ext", None), True)
        kw.update(min_ovlp=min_ovlp, max_ext=max_ext, pairs=True)
        ptrs = []

        def alloc(nbytes):
            ptrs.append(self.dev_alloc(max(int(nbytes), 8)))
            return ptrs[-1]

        def fetch(dev, shape, dtype):
            a = np.zeros(shape, dtype)
            if a.nbytes:
                self.L.rb2_hip_memcpy(self.h, a.ctypes.data, dev, a.nbytes, 1)
            return a
        try:
            cap = 2 * n + 16
            d_edges = alloc(32 * cap)
            m, info = self.string_graph_dev(0, n, d_edges, cap, **kw)
            if m > cap:                                             # (the guess was short: once more with room for all)
                self.dev_free(ptrs.pop())
                cap = m
                d_edges = alloc(32 * cap)
                m, info = self.string_graph_dev(0, n, d_edges, cap, **kw)
            if clean is not None:                                   # (no more rows are kept than came: room for all of them)
                d_raw, d_edges = d_edges, alloc(32 * m)
                m, cinfo = self.graph_clean_dev(n, m, d_raw, d_edges, m, **clean)
                info = (info, cinfo)
            d_vtx, d_cinfo = alloc(32 * n), alloc(32)
            self.unitig_chains_dev(n, m, d_edges, d_vtx, d_cinfo)
            _, tinfo = self.unitig_text_dev(n, d_vtx, None, None, canonical, min_reads)
            cap_u, cap_txt = int(tinfo[0]), int(tinfo[1])
            d_urec, d_txt = alloc(40 * cap_u), alloc(cap_txt)
            if cap_u and cap_txt:
                stored, _ = self.unitig_text_dev(n, d_vtx, d_urec, d_txt, canonical, min_reads, cap_u, cap_txt)
                assert stored == cap_u, (stored, cap_u)
            self.sync()
            urec = fetch(d_urec, (cap_u, 5), np.int64) if cap_txt else np.zeros((0, 5), np.int64)
            txt = fetch(d_txt, cap_txt, np.uint8)
            vtx = fetch(d_vtx, (n, 4), np.int64)[:, :2]            # head and rank: the chain order
            self.sync()
        finally:
            for d in ptrs:
                self.dev_free(d)
        order = np.lexsort((vtx[:, 1], vtx[:, 0]))
        first = np.searchsorted(vtx[order, 0], urec[:, 0])
        return [(txt[o:o + l].copy(), order[f:f + k].copy(), bool(fl & 1)) for (hd, k, o, l, fl), f in zip(urec.tolist(), first.tolist())], info

    # -- measurement helpers ----------------------------------------------------------------
    # -- the strings back out of the index, and one index into another (include/rb2_hip.h) ------------
    def _n_strings(self):
        """strings the index holds: the rows of the $ block"""
        return int(self.counts()[:, 0].sum())

    def unpack_raw(self, first=0, n=None, reversed=False):
        """rb2_hip_unpack: (txt, off) of strings first .. first + n - 1 (n = None: up to the last): txt[off[i]:off[i + 1]] = string first + i
        and one 0, last symbol first when reversed (then txt is a batch insert_multi accepts).  Sizes with one call, fetches with a second"""
        if n is None:
            n = self._n_strings() - first
        off = np.zeros(max(n, 0) + 1, np.int64)
        size = int(self.L.rb2_hip_unpack(self.h, first, n, int(bool(reversed)), 0, None, off.ctypes.data))
        txt = np.empty(size, np.uint8)
        if size:
            got = int(self.L.rb2_hip_unpack(self.h, first, n, int(bool(reversed)), size, txt.ctypes.data, off.ctypes.data))
            assert got == size, (got, size)
        return txt, off

    def unpack(self, first=0, n=None):
        """strings first .. first + n - 1 of the index in text order, one nt6 array each"""
        txt, off = self.unpack_raw(first, n, False)
        return [txt[off[i]:off[i + 1] - 1].copy() for i in range(len(off) - 1)]

    def unpack_dev(self, first, n, reversed, cap, txt_dev, off_dev):
        """rb2_hip_unpack_dev: txt_dev (cap bytes) and off_dev (n + 1 int64) in this device's memory, either may be None; returns SIZE
        behind one synchronise, the text kernel is queued on the handle's stream"""
        return int(self.L.rb2_hip_unpack_dev(self.h, first, n, int(bool(reversed)), cap, txt_dev, off_dev))

    def merge(self, other, batch_bytes=0):
        """rb2_hip_merge: insert every string of `other` (a HipBwt on the same device; unchanged) into this index, in batches of at most
        batch_bytes bytes of text (0: a default from the free memory).  Returns (strings, symbols without sentinels, batches, largest batch)"""
        info = np.zeros(4, np.int64)
        self.L.rb2_hip_merge(self.h, other.h, batch_bytes, info.ctypes.data)
        return tuple(int(v) for v in info)

    # -- reads corrected by the k-mer spectrum of the index (include/rb2_hip.h) -----------------------
    @staticmethod
    def correct_default_probes(reads_len=101, k=21, attempts=32):
        """the default max_probes, by arithmetic and not measured: the profile of a read of reads_len symbols (at most one probe per
        symbol) plus `attempts` tried windows of three alternatives each and the k windows a fix re-evaluates: 101 + 32 * 24 = 869"""
        return int(reads_len) + int(attempts) * (3 + int(k))

    def correct_raw(self, reads, k, min_occ=3, max_fix=8, max_probes=None):
        """rb2_hip_correct as it is: (fixes, out, off, cnt, weak) -- out[off[i]:off[i + 1]] = read i corrected, cnt[i] >= 0 its fixes,
        -1 malformed (copied unchanged), <= -2 over budget with -2 - cnt[i] fixes made; weak[i] = weak positions left (-1 for those two)"""
        qry, off = pack_patterns(reads)
        n = len(off) - 1
        if max_probes is None:
            max_probes = self.correct_default_probes(int(np.diff(off).max(initial=0)), k)
        out = np.zeros(len(qry), np.uint8)
        cnt, weak = np.zeros(n, np.int64), np.zeros(n, np.int64)
        fixes = self.L.rb2_hip_correct(self.h, n, qry.ctypes.data, off.ctypes.data, int(k), int(min_occ), int(max_fix), int(max_probes),
                                       out.ctypes.data, cnt.ctypes.data, weak.ctypes.data)
        return int(fixes), out, off, cnt, weak

    def correct(self, reads, k, min_occ=3, max_fix=8, max_probes=None):
        """the reads (str / bytes over ACGTN, or nt6 arrays) corrected by the k-mer spectrum of the index: (corrected nt6 arrays, cnt,
        weak); a malformed read comes back as it is with cnt = -1.  max_probes = None: correct_default_probes of the longest read.
        Raises StepBudgetExceeded when a read ran over its budget: the exception names the reads and carries the same triple, those
        reads with the fixes made by then"""
        _, out, off, cnt, weak = self.correct_raw(reads, k, min_occ, max_fix, max_probes)
        res = ([out[off[i]:off[i + 1]].copy() for i in range(len(off) - 1)], cnt, weak)
        raise_over_budget(cnt, res, "correct", "max_fix", "max_probes")
        return res

    def correct_dev(self, n, qry_dev, off_dev, total, out_dev, cnt_dev, weak_dev, k, min_occ=3, max_fix=8, max_probes=869):
        """rb2_hip_correct_dev: all five pointers in this device's memory, total >= off[n] - off[0]; out_dev may be qry_dev;
        asynchronous on the handle's stream"""
        self.L.rb2_hip_correct_dev(self.h, n, qry_dev, off_dev, int(total), int(k), int(min_occ), int(max_fix), int(max_probes), out_dev, cnt_dev, weak_dev)

    CORRECT_INFO = ("strings", "changed", "fixes", "weak", "over_budget", "malformed", "batches", "largest_batch")

    def correct_into(self, dst, k, min_occ=3, max_fix=8, max_probes=869, pairs=False, batch_bytes=0):
        """rb2_hip_correct_into: every string of this index corrected against this index and inserted into dst (a HipBwt on the same
        device); this index is unchanged.  pairs: strings 2i and 2i + 1 are a read and its reverse complement, only 2i is corrected.
        Returns the info as a dict (CORRECT_INFO) with the symbols added under the key symbols"""
        info = np.zeros(8, np.int64)
        added = self.L.rb2_hip_correct_into(dst.h, self.h, int(k), int(min_occ), int(max_fix), int(max_probes), int(bool(pairs)), int(batch_bytes), info.ctypes.data)
        d = dict(zip(self.CORRECT_INFO, (int(v) for v in info)))
        d["symbols"] = int(added)
        return d

    def corrected(self, k, min_occ=3, max_fix=8, max_probes=869, pairs=False, batch_bytes=0):
        """a new handle of the same sorting order on the same device that holds this index's strings corrected: (handle, info)"""
        g = HipBwt(self.so, getattr(self, "dev", 0))
        try:
            info = self.correct_into(g, k, min_occ, max_fix, max_probes, pairs, batch_bytes)
        except BaseException:
            g.close()
            raise
        return g, info

    def dev_alloc(self, nbytes):
        return self.L.rb2_hip_dev_alloc(self.h, nbytes)

    def dev_free(self, p):
        self.L.rb2_hip_dev_free(self.h, p)

    def synth_reads(self, dev_ptr, first, n_reads, read_len, seed=42, strand=0, genome_len=0, skew=0):
        self.L.rb2_hip_synth_reads_skew(self.h, dev_ptr, first, n_reads, read_len, seed, strand, genome_len, skew)

    def sync(self):
        self.L.rb2_hip_sync(self.h)

    def sparse_stats(self):
        a = np.zeros(4, np.int64)
        self.L.rb2_hip_sparse_stats(self.h, a.ctypes.data)
        return {"relayouts": int(a[0]), "void_rounds": int(a[1]), "sparse_rounds": int(a[2]), "sparse_now": bool(a[3])}

    def layout_stats(self):
        a = np.zeros(8, np.int64)
        self.L.rb2_hip_layout_stats(self.h, a.ctypes.data)
        return {"relayouts": int(a[0]), "void_rounds": int(a[1]), "sparse_rounds": int(a[2]), "sparse_now": bool(a[3]),
                "respreads": int(a[4]), "leaf_splits": int(a[5]), "grown_in_rounds": int(a[6]), "plain_handovers": int(a[7])}

    def rewind_stats(self):
        """void in-place rounds taken back from behind queued rounds (rb2_hip_rewind_stats)"""
        a = np.zeros(4, np.int64)
        self.L.rb2_hip_rewind_stats(self.h, a.ctypes.data)
        return {"rewinds": int(a[0]), "rounds_taken_back": int(a[1]), "deepest": int(a[2]), "even_depth": int(a[3])}

    def steady_stats(self):
        """rounds of one-member groups (rb2_hip_steady_stats): dense rounds with a k_advance of their own (always 0: measured, not kept) / without a
        k_prep launch since create; the round of the last batch the device first reported the state at and the one the host used it from (-1: never)"""
        a = np.zeros(4, np.int64)
        self.L.rb2_hip_steady_stats(self.h, a.ctypes.data)
        return {"advance_single": int(a[0]), "prep_skipped": int(a[1]), "reported_at": int(a[2]), "used_from": int(a[3])}

    def lean_stats(self):
        """lean rounds (rb2_hip_lean_stats): dense rounds run without an insert list since create / the stage in force (0: off; 2 once a lean round
        with the three-launch counting tail has been queued, 1 until then; RB2_STEADY_LEAN)"""
        a = np.zeros(2, np.int64)
        self.L.rb2_hip_lean_stats(self.h, a.ctypes.data)
        return {"rounds": int(a[0]), "stage": int(a[1])}

    def lean_count_stats(self):
        """stage 2 of the lean round (rb2_hip_lean_count_stats): rounds counted by k_count_lean since create / audit rounds (counted by k_sym as in
        stage 1; RB2_LEAN_AUDIT) / rounds in which both ways ran and were compared (RB2_LEAN_VERIFY=1) / words in which they differed"""
        a = np.zeros(4, np.int64)
        self.L.rb2_hip_lean_count_stats(self.h, a.ctypes.data)
        return {"counted": int(a[0]), "audit": int(a[1]), "verified": int(a[2]), "mismatches": int(a[3])}

    def lean_fork_stats(self):
        """the forked round (rb2_hip_lean_fork_stats): rounds whose counting tail ran on the side stream beside their merge since create / whether
        such rounds are forked (RB2_LEAN_FORK, default 1; never on a caller's stream or with RB2_LEAN_VERIFY)"""
        a = np.zeros(2, np.int64)
        self.L.rb2_hip_lean_fork_stats(self.h, a.ctypes.data)
        return {"forked": int(a[0]), "on": int(a[1])}

    def lean_dir_stats(self):
        """the window directory (rb2_hip_lean_dir_stats): lean rounds that kept the rank directory of the side they wrote per window since create /
        the switch (RB2_LEAN_DIR, default 1) / the lean rounds that were allowed to write compact windows, whatever the switch says"""
        a = np.zeros(3, np.int64)
        self.L.rb2_hip_lean_dir_stats(self.h, a.ctypes.data)
        return {"rounds": int(a[0]), "on": int(a[1]), "lean_compact": int(a[2])}

    def window_stats(self):
        a = np.zeros(6, np.int64)
        self.L.rb2_hip_window_stats(self.h, a.ctypes.data)
        return {"plain": int(a[0]), "compact0": int(a[1]), "compact1": int(a[2]), "compact2": int(a[3]), "compact_rounds": int(a[4]), "counted": bool(a[5])}

    def profile(self, on=True):
        """False / 0: off; True / 1: every kernel group of a round; 2: the merge launches only (two events per round instead of sixteen)"""
        self.L.rb2_hip_profile(self.h, int(on))

    def profile_get(self, reset=False):
        n = len(K_NAMES)
        la = np.zeros(n, np.int64)
        ms = np.zeros(n, np.float64)
        un = np.zeros(n, np.int64)
        self.L.rb2_hip_profile_get(self.h, la.ctypes.data, ms.ctypes.data, un.ctypes.data, 1 if reset else 0)
        return {K_NAMES[i]: {"launches": int(la[i]), "ms": float(ms[i]), "units": int(un[i])} for i in range(n)}

    SCAN_OPS = {"add32": 0, "add64": 1, "sat": 2, "max": 3}
    SCAN_FORMS = {"multi": 0, "block256": 1, "block1024": 2}

    def scan_check(self, op, form, values):
        """one of the engine's cold-path prefix scans (rb2_hip_scan_check) over values: (out[0 .. n], the block prefixes, the total word, items per block)"""
        x = np.ascontiguousarray(values, np.uint64)
        out = np.zeros(len(x) + 1, np.uint64)
        parts = np.zeros(len(x) // 256 + 2, np.uint64)
        tot = np.zeros(1, np.uint64)
        per = int(self.L.rb2_hip_scan_check(self.h, self.SCAN_OPS[op], self.SCAN_FORMS[form], len(x), x.ctypes.data, out.ctypes.data, parts.ctypes.data, tot.ctypes.data))
        return out, parts[:(len(x) + per - 1) // per] if form == "multi" else None, int(tot[0]), per

    @staticmethod
    def layout():
        L = load_hip_lib()
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        L.rb2_hip_layout(C.byref(a), C.byref(b), C.byref(c))
        return {"leaf_syms": a.value, "tile_leaves": b.value, "string_tile": c.value}


TRANSPORTS = {"peer": 0, "rccl": 1}


class _Engine(HipBwt):
    """a local rank's engine inside a MultiBwt (borrowed handle: never destroyed from here)"""

    def __init__(self, lib, h, so):
        self.L, self.h, self.so = lib, h, so

    def close(self):
        self.h = None


class MultiBwt:
    """One BWT whose 31 sub-ropes are sharded over N ranks, driven inside the library (include/rb2_hip.h, rb2_hip_multi_*):
    the same ``insert_multi(buf)`` contract as ``HipBwt`` / mr_insert_multi (mrope.c:258), no Python in the round loop.

    ``devices``: one entry per rank; the same device may appear several times (virtual ranks on one GPU, PEER transport).
    ``rank``/``nranks``/``nccl_id``: this process is ONE rank of a multi-process group over RCCL (bench.py under torchrun)."""

    def __init__(self, sorting_order, devices, transport="peer", owners=None, rank=None, nranks=None, nccl_id=None):
        self.L = load_hip_lib()
        if self.L.rb2_hip_device_count() <= 0:
            raise RuntimeError("no HIP device visible: the gfx950 engine has no CPU fallback")
        own = (C.c_int * len(owners))(*owners) if owners is not None else None
        self.so = sorting_order
        if rank is None:
            devs = (C.c_int * len(devices))(*devices)
            self.h = self.L.rb2_hip_multi_create(len(devices), devs, sorting_order, TRANSPORTS[transport], own)
        else:
            idb = C.create_string_buffer(bytes(nccl_id), 128) if nccl_id is not None else None
            self.h = self.L.rb2_hip_multi_create_rank(devices[0], rank, nranks, idb, sorting_order, own)
        self.n = self.L.rb2_hip_multi_nlocal(self.h)
        self.world = self.L.rb2_hip_multi_nranks(self.h)

    @staticmethod
    def unique_id():
        b = C.create_string_buffer(128)
        load_hip_lib().rb2_hip_multi_unique_id(b)
        return b.raw

    @staticmethod
    def default_owners(nranks):
        a = (C.c_int * 31)()
        load_hip_lib().rb2_hip_default_owners(nranks, a)
        return list(a)

    def text_bytes(self):
        """bytes of device memory every local rank holds for the text of the last host-buffer batch (rb2_hip_multi_text_bytes)"""
        return [int(self.L.rb2_hip_multi_text_bytes(self.h, k)) for k in range(self.n)]

    def close(self):
        if getattr(self, "h", None):
            self.L.rb2_hip_multi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def engine(self, k=0):
        return _Engine(self.L, self.L.rb2_hip_multi_engine(self.h, k), self.so)

    def insert_multi(self, buf):
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        self.L.rb2_hip_multi_insert_multi(self.h, len(buf), buf.ctypes.data)

    def insert_multi_dev(self, dev_ptrs, nbytes):
        """dev_ptrs: one device pointer per local rank (or a single pointer all local ranks share)"""
        if not isinstance(dev_ptrs, (list, tuple)):
            dev_ptrs = [dev_ptrs] * self.n
        arr = (C.c_void_p * self.n)(*dev_ptrs)
        self.L.rb2_hip_multi_insert_multi_dev(self.h, nbytes, arr)

    def counts(self):
        c = np.zeros(36, np.int64)
        self.L.rb2_hip_multi_get_counts(self.h, c.ctypes.data)
        return c.reshape(6, 6)

    def rope_rle(self, b):
        n = self.L.rb2_hip_multi_rope_bytes(self.h, b)
        out = np.zeros(max(n, 1), np.uint8)
        got = self.L.rb2_hip_multi_download_rope(self.h, b, out.ctypes.data)
        assert got == n
        return out[:n]

    def rope(self, b):
        return expand_runs(self.rope_rle(b))

    def load_ropes(self, rles):
        arrs = [np.ascontiguousarray(r, dtype=np.uint8) for r in rles]
        ptrs = (C.c_void_p * 6)(*[a.ctypes.data if len(a) else None for a in arrs])
        lens = (C.c_int64 * 6)(*[len(a) for a in arrs])
        self.L.rb2_hip_multi_load_ropes(self.h, ptrs, lens)

    def load_fmd(self, src):
        """rb2_hip_multi_load_fmd: every rank decodes the image and keeps its own pieces; src as for HipBwt.load_fmd"""
        img = _fmd_image(src)
        return int(self.L.rb2_hip_multi_load_fmd(self.h, img.ctypes.data, len(img)))

    def reserve(self, batch_bytes=0, batch_strings=0, total_symbols=0):
        self.L.rb2_hip_multi_reserve(self.h, batch_bytes, batch_strings, total_symbols)

    def reset(self):
        self.L.rb2_hip_multi_reset(self.h)

    def rope_hashes(self):
        return [int(self.L.rb2_hip_multi_rope_hash(self.h, b)) for b in range(6)]

    def sync(self):
        self.L.rb2_hip_multi_sync(self.h)

    def rank1a(self, b, x):
        c = np.zeros(6, np.int64)
        self.L.rb2_hip_multi_rank1a(self.h, b, x, c.ctypes.data)
        return c

    def stats(self):
        a = np.zeros(6, np.int64)
        self.L.rb2_hip_multi_stats(self.h, a.ctypes.data)
        return {"host_syncs_in_rounds": int(a[0]), "rounds": int(a[1]), "batches": int(a[2]), "sparse_rounds": int(a[3]),
                "void_rounds": int(a[4]), "relayouts": int(a[5])}
