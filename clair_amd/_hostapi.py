"""ctypes binding of include/clair_host.h (libclair_host.so, built by clair_amd/build.py with g++: no GPU involved)."""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libclair_host.so")
vp, cp, i32, i64, f64 = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
p_vp, p_i32, p_i64 = ctypes.POINTER(vp), ctypes.POINTER(i32), ctypes.POINTER(i64)


def _sig(*argtypes, **kw):
    """One row of SIGNATURES: (restype, argtypes); a function returns int unless restype= says otherwise."""
    return kw.get("restype", i32), list(argtypes)


_DECODE_ROWS = (vp, vp, vp, vp, vp, cp, vp, i32, i32, i32, i32, i32, i32, vp, i64, p_i64, p_i32)
_FEED = (vp, vp, i64, i32, p_i64)
# every function include/clair_host.h declares, with its prototype there as ctypes states it (tests/test_host.py checks header <-> this table
# <-> .so): the one place to add an entry point
SIGNATURES = {
    "clair_host_abi_version": _sig(),
    "clair_host_last_error": _sig(restype=cp),
    "clair_host_threads": _sig(i32),
    "clair_host_crc32c": _sig(cp, i64, restype=ctypes.c_uint32),
    "clair_host_counts_to_input_i16": _sig(vp, i64, vp),
    "clair_host_counts_to_input_i32": _sig(vp, i64, vp),
    "clair_host_parse_tensors": _sig(vp, i64, i32, i32, vp, vp, p_i32, p_i32, p_i64),
    "clair_host_decode_rows": _sig(*_DECODE_ROWS),
    "clair_host_decode_rows_ex": _sig(*_DECODE_ROWS + (vp,)),
    "clair_host_resolve_calls": _sig(vp, vp, vp, vp, vp, vp, i32, vp),
    "clair_host_format_calls": _sig(vp, cp, vp, i32, i32, i32, i32, i32, i32, vp, i64, p_i64, p_i32, vp),
    "clair_host_centre_bytes": _sig(cp, vp, i32, vp),
    "clair_host_format_calls_records": _sig(vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, i64, p_i64, p_i32, vp),
    "clair_host_pileup_create": _sig(cp, i64, i64, vp, i64, i32, i32, i32, i32, i64, i32, p_vp),
    "clair_host_pileup_destroy": _sig(vp, restype=None),
    "clair_host_pileup_set_order": _sig(vp, i32),
    "clair_host_pyset_order": _sig(vp, i64, vp, i64, p_i64),
    "clair_host_pileup_feed": _sig(*_FEED),
    "clair_host_pileup_finish": _sig(vp),
    "clair_host_pileup_pending": _sig(vp, restype=i64),
    "clair_host_pileup_take": _sig(vp, i64, vp, vp, vp, p_i64),
    "clair_host_pileup_take_text": _sig(vp, cp, vp, i64, p_i64, p_i64),
    "clair_host_pileup_stats": _sig(vp, vp),
    "clair_host_evc_create": _sig(cp, cp, i64, i64, i64, i64, vp, vp, i64, f64, f64, i32, p_vp),
    "clair_host_evc_destroy": _sig(vp, restype=None),
    "clair_host_evc_feed": _sig(*_FEED),
    "clair_host_evc_finish": _sig(vp),
    "clair_host_evc_pending": _sig(vp, restype=i64),
    "clair_host_evc_reads": _sig(vp, restype=i64),
    "clair_host_evc_take": _sig(vp, i64, vp, p_i64),
    "clair_host_evc_take_text": _sig(vp, vp, i64, p_i64, p_i64),
    "clair_host_sampack_create": _sig(cp, i32, i32, i32, i64, i64, p_vp),
    "clair_host_sampack_destroy": _sig(vp, restype=None),
    "clair_host_sampack_feed": _sig(*_FEED),
    "clair_host_sampack_stats": _sig(vp, vp),
    "clair_host_sampack_slab": _sig(vp, p_vp, p_vp, p_vp, p_vp),
    "clair_host_sampack_reset": _sig(vp),
    "clair_host_sampack_set_lookup": _sig(vp, i32),
    "clair_host_indel_table": _sig(vp, vp, vp, vp, vp, vp, i64, vp, i64, vp, i32, vp, vp, vp),
    "clair_host_tuple_budget_binds": _sig(vp, vp, i64, vp, vp, i64, vp, p_i32),
    "clair_host_bam_open": _sig(cp, i32, p_vp),
    "clair_host_bam_close": _sig(vp, restype=None),
    "clair_host_bam_info": _sig(vp, vp),
    "clair_host_bam_ref": _sig(vp, i32, ctypes.POINTER(cp), p_i64),
    "clair_host_bam_tid": _sig(vp, cp),
    "clair_host_bam_query": _sig(vp, cp, i32, i64, i64),
    "clair_host_bam_next": _sig(vp, vp, i64, vp, i64, p_i64, p_i64),
    "clair_host_bam_voffset": _sig(vp, i64, ctypes.POINTER(ctypes.c_uint64)),
    "clair_host_bam_render": _sig(vp, vp, vp, i64, i32, i64, i64, p_vp, p_i64),
    "clair_host_faidx": _sig(cp, cp, i64, i64, vp, i64, p_i64),
    "clair_host_bam_set_inflater": _sig(vp, vp, vp, i32),
    "clair_host_bam_set_subsample": _sig(vp, i64, f64),
    "clair_host_subsample_keeps": _sig(vp, i64, i64, f64),
    "clair_host_inflate_block": _sig(vp, i64, vp, i64, p_i64, ctypes.POINTER(ctypes.c_uint32), p_i32),
    "clair_host_inflate_bgzf": _sig(vp, i64, vp, p_i64, p_i32),
    "clair_host_deflate_bgzf": _sig(vp, i64, vp, p_i64),
    "clair_host_ensemble_average": _sig(vp, i32, i64, vp),
    "clair_host_ensemble_quantise": _sig(vp, i64, vp),
    "clair_host_ensemble_value": _sig(vp, i64, vp),
    "clair_host_overlap_keep": _sig(vp, i64, vp),
    "clair_host_train_set_key": _sig(cp, i64, i32, p_i64),
    "clair_host_train_set_sample": _sig(vp, i64, vp, i64, f64, f64, i64, vp, vp, vp, p_i64, p_i64),
    "clair_host_train_set_pair_count": _sig(vp, i64, vp, i64, vp, vp, i64, p_i64, p_i64),
    "clair_host_train_set_ratio": _sig(i64, f64, i64, ctypes.POINTER(f64)),
    "clair_host_train_set_pair_keep": _sig(vp, i64, vp, i64, vp, vp, i64, f64, i64, vp, p_i64, p_i64),
    "clair_host_train_set_labels": _sig(vp, vp, i64, vp, vp, i64, vp, vp, i64, vp, vp),
    "clair_host_sites_create": _sig(p_vp),
    "clair_host_sites_destroy": _sig(vp, restype=None),
    "clair_host_sites_begin_source": _sig(vp, vp, i64, p_i64),
    "clair_host_sites_add_rows": _sig(vp, i64, vp, i64, vp, vp, vp),
    "clair_host_sites_finish": _sig(vp, i32, i32, p_i64),
    "clair_host_sites_info": _sig(vp, i64, i64, vp, vp, vp),
    "clair_host_sites_rows": _sig(vp, i64, i64, vp),
    "clair_host_sites_windows": _sig(vp, i64, i64, vp),
    "clair_host_compare_create": _sig(p_vp),
    "clair_host_compare_destroy": _sig(vp, restype=None),
    "clair_host_compare_set_contigs": _sig(vp, vp, vp, i32),
    "clair_host_compare_set_regions": _sig(vp, vp, vp, vp, i64),
    "clair_host_compare_parse": _sig(vp, i32, vp, i64, vp),
    "clair_host_compare_keys": _sig(vp, i32, vp),
    "clair_host_compare_permute": _sig(vp, i32, vp),
    "clair_host_compare_run": _sig(vp),
    "clair_host_compare_counts": _sig(vp, vp),
    "clair_host_compare_records": _sig(vp, i32, vp, vp),
    "clair_host_compare_set_reference": _sig(vp, vp, vp, i32),
    "clair_host_compare_left_align": _sig(vp, i32, vp),
    "clair_host_compare_allele_text": _sig(vp, i32, vp),
    "clair_host_bamidx_create": _sig(i32, i32, i32, p_vp),
    "clair_host_bamidx_destroy": _sig(vp, restype=None),
    "clair_host_bamidx_begin": _sig(vp, i32, vp),
    "clair_host_bamidx_batch": _sig(vp, vp, i64, i32, vp, vp, vp, vp, i64, i64, i32, vp, p_vp),
    "clair_host_bamidx_finish": _sig(vp, vp, i64, vp),
    "clair_host_bamidx_backend": _sig(vp, vp),
    "clair_host_bamidx_debug_frame": _sig(vp, i64, i64, i32, vp, i64, vp),
    "clair_host_bamidx_build": _sig(cp, vp, i32, p_vp),
    "clair_host_bamidx_result_info": _sig(vp, vp),
    "clair_host_bamidx_result_copy": _sig(vp, vp, vp, vp),
    "clair_host_bamidx_result_free": _sig(vp, restype=None),
    "clair_host_bam_job_open": _sig(cp, p_vp),
    "clair_host_bam_job_close": _sig(vp, restype=None),
    "clair_host_bam_job_header": _sig(vp, vp, i64, p_i64),
    "clair_host_bamsort_create": _sig(i32, i32, i32, p_vp),
    "clair_host_bamsort_destroy": _sig(vp, restype=None),
    "clair_host_bamsort_begin": _sig(vp, i32, vp, i64),
    "clair_host_bamsort_pass": _sig(vp, i64, i64, i32),
    "clair_host_bamsort_batch": _sig(vp, vp, i64, i32, vp, vp, vp, vp, i64, i64, i32, vp),
    "clair_host_bamsort_histogram": _sig(vp, vp, i64),
    "clair_host_bamsort_sort": _sig(vp, i32, vp),
    "clair_host_bamsort_emit": _sig(vp, i64, i32, i32, vp, vp),
    "clair_host_bamsort_backend": _sig(vp, vp),
    "clair_host_bamsort_debug_sort": _sig(vp, i64, vp),
    "clair_host_bamsort_debug_gather": _sig(vp, i64, vp, vp, i64, vp, i64),
    "clair_host_bamsort_run": _sig(vp, vp, cp, i32, i64, i32, i32, vp),
    "clair_host_markdup_create": _sig(i32, i32, i32, p_vp),
    "clair_host_markdup_destroy": _sig(vp, restype=None),
    "clair_host_markdup_begin": _sig(vp, i32, i64, i32),
    "clair_host_markdup_batch": _sig(vp, vp, i64, i32, vp, vp, vp, vp, i64, i64, i32, vp),
    "clair_host_markdup_resolve": _sig(vp),
    "clair_host_markdup_mark": _sig(vp, vp, i64, i32, vp, vp, vp, vp, i64, i64, i32, vp),
    "clair_host_markdup_emit": _sig(vp, i64, i32, i32, vp, vp),
    "clair_host_markdup_stats": _sig(vp, vp),
    "clair_host_markdup_backend": _sig(vp, vp),
    "clair_host_markdup_debug_summary": _sig(vp, i64, vp, i64, i32, vp),
    "clair_host_markdup_debug_resolve": _sig(vp, i64, vp),
    "clair_host_markdup_run": _sig(vp, vp, cp, i32, i64, i32, i32, i32, vp),
    "clair_host_gvcf_tally": _sig(vp, i64, vp, i64, vp, i64, i64, i64, vp, vp),
    "clair_host_gvcf_blocks": _sig(vp, i64, i64, vp, i64, i64, i32, i32, i32, vp, vp, vp, i64, vp, i64, p_i64),
    "clair_host_gvcf_format": _sig(vp, i64, i64, cp, vp, i64, i64, vp, i64, p_i64, vp),
}
SYMBOLS = tuple(SIGNATURES)
N_VALUES = 1056
_lib = None


def load():
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise RuntimeError("%s not found: run `python -m clair_amd.build`" % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
        if lib.clair_host_abi_version() != 6:
            raise RuntimeError("libclair_host.so has ABI version %d, expected 6: run `python -m clair_amd.build`"
                               % lib.clair_host_abi_version())
        _lib = lib
    return _lib


class Handle(object):
    """One native handle and the two functions of its library that go with it.  A subclass calls _own() and hands what it returns to its create
    function; close() may be repeated, __del__ never raises, _check() turns a non-zero return code into the subclass's exception."""
    _h = None
    _error = ValueError

    def _own(self, destroy, last_error):
        self._destroy, self._last_error = destroy, last_error
        self._h = ctypes.c_void_p()
        return ctypes.byref(self._h)

    def _check(self, rc, what=""):
        if rc != 0:
            raise self._error(what + self._last_error().decode())

    def close(self):
        if self._h:
            self._destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def crc32c(data):
    """CRC32C (Castagnoli) of a bytes object."""
    return int(load().clair_host_crc32c(data, len(data)))


def counts_to_input(counts):
    """Raw pileup counts [n,33,8,4] (int16 or int32) -> float32 network input with channels 1..3 -= channel 0 (utils.py:96-98)."""
    lib = load()
    c = np.ascontiguousarray(counts)
    if c.dtype not in (np.int16, np.int32):
        c = c.astype(np.int32)
    x = np.empty(c.shape, dtype=np.float32)
    fn = lib.clair_host_counts_to_input_i16 if c.dtype == np.int16 else lib.clair_host_counts_to_input_i32
    if fn(c.ctypes.data, c.size // 4, x.ctypes.data) != 0:
        raise ValueError("counts_to_input: " + lib.clair_host_last_error().decode())
    return x


class MetaInfoTable(object):
    """The [[ctg, pos, seq], ...] list of a batch of text records, kept as the bytes the parser found them in: `meta` holds the
    three fields of every candidate back to back, tok[i] = (offset, length) x 3 into it -- the form clair_host_decode_rows takes, so
    a batch reaches the native decoder without a Python string per field.  List-like: len, iteration, indexing and comparison give
    the lists of three strings."""

    def __init__(self, meta, tok):
        self.meta, self.tok = meta, tok
        self._rows = None

    @classmethod
    def from_chunk(cls, chunk, tok):
        """Compact the fields tok points at inside `chunk` (a parse buffer of megabytes) into their own small buffer."""
        k = len(tok)
        lens = tok[:, 1::2].astype(np.int64).ravel()
        starts = tok[:, 0::2].astype(np.int64).ravel()
        before = np.cumsum(lens) - lens
        index = np.repeat(starts - before, lens) + np.arange(int(lens.sum()), dtype=np.int64)
        meta = np.frombuffer(chunk, dtype=np.uint8)[index].tobytes()
        out = np.empty((k, 6), dtype=np.int32)
        out[:, 0::2] = before.reshape(k, 3)
        out[:, 1::2] = lens.reshape(k, 3)
        return cls(meta, out)

    @classmethod
    def concat(cls, tables):
        tables = [t for t in tables if len(t)]
        if len(tables) == 1:
            return tables[0]
        if not tables:
            return cls(b"", np.zeros((0, 6), dtype=np.int32))
        shift, toks = 0, []
        for t in tables:
            tk = t.tok.copy()
            tk[:, 0::2] += shift
            toks.append(tk)
            shift += len(t.meta)
        return cls(b"".join(t.meta for t in tables), np.concatenate(toks))

    def __len__(self):
        return len(self.tok)

    def rows(self):
        if self._rows is None:
            m = self.meta
            self._rows = [[m[o[0]:o[0] + o[1]].decode(), m[o[2]:o[2] + o[3]].decode(), m[o[4]:o[4] + o[5]].decode()] for o in self.tok.tolist()]
        return self._rows

    def __getitem__(self, i):
        return self.rows()[i]

    def __iter__(self):
        return iter(self.rows())

    def __eq__(self, other):
        return self.rows() == (other.rows() if hasattr(other, "rows") else other)

    def native_meta(self):
        return self.meta, self.tok


def parse_tensors(chunk, final, max_rows, x_out, row0, offset=0):
    """Parse up to max_rows lines of `chunk` (bytes), starting at byte `offset`, into x_out[row0:] (float32 [*,1056],
    C-contiguous).  -> (rows_taken, infos of the kept rows as a MetaInfoTable ([[ctg, pos, seq], ...]), bytes_consumed)"""
    lib = load()
    tok = np.empty((max(max_rows, 1), 6), dtype=np.int32)
    taken, kept, used = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0)
    base = ctypes.cast(ctypes.c_char_p(chunk), ctypes.c_void_p).value      # bytes: passed by pointer, no copy
    rc = lib.clair_host_parse_tensors(base + offset, len(chunk) - offset, 1 if final else 0, max_rows,
                                      x_out[row0:].ctypes.data, tok.ctypes.data,
                                      ctypes.byref(taken), ctypes.byref(kept), ctypes.byref(used))
    if rc != 0:
        raise ValueError("malformed tensor record: " + lib.clair_host_last_error().decode())
    t = tok[:kept.value].astype(np.int64)
    t[:, 0::2] += offset
    return taken.value, MetaInfoTable.from_chunk(chunk, t), used.value


def decode_rows(X, infos, Y, show_reference, haploid_precision, haploid_sensitive, qual_threshold, arith_numpy2, with_status=False):
    """clair_host_decode_rows over one batch -> list of VCF row strings (input order, skipped candidates left out).
    with_status: also the per-candidate status bytes of clair_host_decode_rows_ex (bit 0: produced a row, bit 1: passed a
    point where the reference would consult the BAM) -> (rows, status uint8 [n])."""
    lib = load()
    n = len(infos)
    if n == 0:
        return ([], np.zeros(0, np.uint8)) if with_status else []
    x = np.ascontiguousarray(X, dtype=np.float32).reshape(n, N_VALUES)
    gt21, genotype, len1, len2 = [np.ascontiguousarray(a, dtype=np.float32) for a in Y]
    meta, tok = _meta_of(infos)
    cap = 4096 + 256 * n + 2 * len(meta)
    out = ctypes.create_string_buffer(cap)
    out_len, n_rows = ctypes.c_int64(0), ctypes.c_int(0)
    status = np.zeros(n, dtype=np.uint8)
    rc = lib.clair_host_decode_rows_ex(x.ctypes.data, gt21.ctypes.data, genotype.ctypes.data, len1.ctypes.data, len2.ctypes.data,
                                       meta, tok.ctypes.data, n, int(bool(show_reference)), int(bool(haploid_precision)),
                                       int(bool(haploid_sensitive)), -1 if qual_threshold is None else int(qual_threshold),
                                       int(bool(arith_numpy2)), out, cap, ctypes.byref(out_len), ctypes.byref(n_rows),
                                       status.ctypes.data)
    if rc != 0:
        raise ValueError("native decode: " + lib.clair_host_last_error().decode())
    rows = out.raw[:out_len.value - 1].decode("ascii").split("\n") if out_len.value else []
    return (rows, status) if with_status else rows


CALL_DTYPE = np.dtype([("status", "u1"), ("family", "u1"), ("index", "<u2"), ("flags", "<u2"), ("gt", "u1"), ("gi", "u1"),
                       ("alt_b0", "u1"), ("alt_b1", "u1"), ("ins_avail", "u1"), ("reserved0", "u1"), ("ins_code", "<u4"),
                       ("depth", "<f4"), ("support", "<f4"), ("p_call", "<f4"), ("rounds", "<u4")])      # include/clair_call.h
assert CALL_DTYPE.itemsize == 32


def _meta_of(infos):
    """(meta bytes, tok int32 [n,6]) of a batch's [[ctg, pos, seq], ...] -- the layout the native decode functions take."""
    n = len(infos)
    if hasattr(infos, "native_meta"):          # tensor_binary.InfoTable / MetaInfoTable: the record columns as they are
        return infos.native_meta()
    parts = [s for info in infos for s in (info[0], str(info[1]), info[2])]
    lens = np.fromiter(map(len, parts), dtype=np.int32, count=3 * n)
    tok = np.empty((n, 6), dtype=np.int32)
    tok[:, 1::2] = lens.reshape(n, 3)
    starts = np.cumsum(lens, dtype=np.int64) - lens
    tok[:, 0::2] = starts.reshape(n, 3)
    return "".join(parts).encode("ascii"), tok


def centre_bytes(infos):
    """uint8 [n,2]: the centre character of every candidate's reference window and min(window length, 255) -- what the call
    resolution needs of the candidate's text (clair_host_resolve_calls, clair_submit_ex)."""
    if hasattr(infos, "centre_bytes"):          # tensor_binary.InfoTable: straight from the record columns
        return infos.centre_bytes()
    lib = load()
    n = len(infos)
    meta, tok = _meta_of(infos)
    out = np.zeros((n, 2), dtype=np.uint8)
    if n and lib.clair_host_centre_bytes(meta, tok.ctypes.data, n, out.ctypes.data) != 0:
        raise ValueError("native decode: " + lib.clair_host_last_error().decode())
    return out


def resolve_calls(X, Y, centre):
    """clair_host_resolve_calls: the arithmetic half of the decode on the CPU -> structured array of call records (CALL_DTYPE)."""
    lib = load()
    n = len(centre)
    calls = np.zeros(n, dtype=CALL_DTYPE)
    if n == 0:
        return calls
    x = np.ascontiguousarray(X, dtype=np.float32).reshape(n, N_VALUES)
    gt21, genotype, len1, len2 = [np.ascontiguousarray(a, dtype=np.float32) for a in Y]
    c = np.ascontiguousarray(centre, dtype=np.uint8)
    if lib.clair_host_resolve_calls(x.ctypes.data, gt21.ctypes.data, genotype.ctypes.data, len1.ctypes.data, len2.ctypes.data,
                                    c.ctypes.data, n, calls.ctypes.data) != 0:
        raise ValueError("native decode: " + lib.clair_host_last_error().decode())
    return calls


def format_calls(calls, infos, show_reference, haploid_precision, haploid_sensitive, qual_threshold, arith_numpy2, with_status=False, as_text=False):
    """clair_host_format_calls: call records (from the GPU decode kernel or resolve_calls) + the batch's text -> VCF rows (a list of
    strings; as_text=True: the rows as one bytes object, each '\\n'-terminated, ready for the file).  A batch of binary tensor records
    (tensor_binary.InfoTable) hands its columns over as they are (clair_host_format_calls_records)."""
    lib = load()
    n = len(infos)
    if n == 0:
        empty = b"" if as_text else []
        return (empty, np.zeros(0, np.uint8)) if with_status else empty
    calls = np.ascontiguousarray(calls, dtype=CALL_DTYPE)
    if len(calls) != n:
        raise ValueError("%d call records for %d candidates" % (len(calls), n))
    flags = (int(bool(show_reference)), int(bool(haploid_precision)), int(bool(haploid_sensitive)),
             -1 if qual_threshold is None else int(qual_threshold), int(bool(arith_numpy2)))
    out_len, n_rows = ctypes.c_int64(0), ctypes.c_int(0)
    status = np.zeros(n, dtype=np.uint8)
    if hasattr(infos, "record_columns"):
        ctg, ctg_len, pos, seq, seq_len = infos.record_columns()
        cap = 4096 + 320 * n
        out = ctypes.create_string_buffer(cap)
        rc = lib.clair_host_format_calls_records(calls.ctypes.data, ctg.ctypes.data, ctg_len.ctypes.data, pos.ctypes.data, seq.ctypes.data,
                                                 seq_len.ctypes.data, n, *flags, out, cap, ctypes.byref(out_len), ctypes.byref(n_rows),
                                                 status.ctypes.data)
    else:
        meta, tok = _meta_of(infos)
        cap = 4096 + 256 * n + 2 * len(meta)
        out = ctypes.create_string_buffer(cap)
        rc = lib.clair_host_format_calls(calls.ctypes.data, meta, tok.ctypes.data, n, *flags, out, cap, ctypes.byref(out_len), ctypes.byref(n_rows),
                                         status.ctypes.data)
    if rc != 0:
        raise ValueError("native decode: " + lib.clair_host_last_error().decode())
    if as_text:
        rows = out.raw[:out_len.value]
    else:
        rows = out.raw[:out_len.value - 1].decode("ascii").split("\n") if out_len.value else []
    return (rows, status) if with_status else rows


def pyset_order(ops):
    """Iteration order of CPython's set after a history of operations (key >= 0: add, -(key + 1): remove), by the native restatement."""
    lib = load()
    ops = np.ascontiguousarray(ops, dtype=np.int64)
    keys = np.empty(max(len(ops), 1), np.int64)
    n = ctypes.c_int64(0)
    if lib.clair_host_pyset_order(ops.ctypes.data, len(ops), keys.ctypes.data, len(keys), ctypes.byref(n)) != 0:
        raise ValueError(lib.clair_host_last_error().decode())
    return keys[:n.value].tolist()


class _LineSink(Handle):
    """A native consumer of `samtools view` text.  A subclass sets _lib, _h (its handle) and _feed (its clair_host_*_feed)."""

    def feed(self, sam, final=False):
        """Consume complete lines of `sam` (bytes or str); returns the unconsumed tail (same type)."""
        data = sam.encode("latin-1") if isinstance(sam, str) else sam
        used = ctypes.c_int64(0)
        base = ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p).value
        if self._feed(self._h, base, len(data), 1 if final else 0, ctypes.byref(used)) != 0:
            from .create_tensor import PileupError
            raise PileupError(self._lib.clair_host_last_error().decode())
        return sam[used.value:]

    def finish(self):
        """Nothing is held back between lines unless the subclass says so."""


def feed_stream(sink, read, chunk_bytes):
    """Feed a SAM stream to a _LineSink, read(chunk_bytes) at a time (bytes or str; empty at the end), whole lines only: what a chunk ends with
    goes in front of the next.  Yields after every feed for the caller to take what has become ready: False after a chunk, True once, after
    the last line (with or without its line end) and finish()."""
    tail = None
    while True:
        chunk = read(chunk_bytes)
        if not chunk:
            break
        tail = sink.feed(chunk if tail is None else tail + chunk)
        yield False
    if tail:
        sink.feed(tail, final=True)
    sink.finish()
    yield True


class PileupBuilder(_LineSink):
    """clair_host_pileup_*: the native twin of clair_amd.create_tensor.PileupBuilderPy (same constructor, same records)."""

    def __init__(self, ctg_name, reference_sequence, reference_start_0_based, candidates, consider_left_edge=True,
                 dcov=250, min_coverage=0, min_mq=0, available_slots=5000000, force_general_path=False, set_order="ascending"):
        if set_order not in ("ascending", "cpython"):
            raise ValueError("set_order: 'ascending' or 'cpython'")
        self._lib = load()
        self.ctg = ctg_name
        ref = reference_sequence.encode("latin-1") if isinstance(reference_sequence, str) else bytes(reference_sequence)
        cands = np.ascontiguousarray(candidates, dtype=np.int64)
        out = self._own(self._lib.clair_host_pileup_destroy, self._lib.clair_host_last_error)
        self._check(self._lib.clair_host_pileup_create(ref, len(ref), int(reference_start_0_based), cands.ctypes.data, len(cands),
                                                       int(bool(consider_left_edge)), int(dcov), int(min_coverage), int(min_mq),
                                                       int(available_slots), int(bool(force_general_path)), out), "pileup: ")
        self._feed = self._lib.clair_host_pileup_feed
        self._text = None
        if set_order == "cpython":
            self._check(self._lib.clair_host_pileup_set_order(self._h, 1), "pileup: ")

    def finish(self):
        self._lib.clair_host_pileup_finish(self._h)

    def pending(self):
        return int(self._lib.clair_host_pileup_pending(self._h))

    def take_arrays(self, max_rows=None):
        """-> (centres int64 [n], refseq list of str, counts int32 [n,33,8,4])"""
        centres, seqs, counts = self.take_columns(max_rows)
        raw = seqs.tobytes()
        return centres, [raw[i * 34:i * 34 + 34].split(b"\0", 1)[0].decode("latin-1") for i in range(len(centres))], counts

    def take_columns(self, max_rows=None):
        """take_arrays without a Python string per window: -> (centres int64 [n], refseq bytes uint8 [n,34] NUL-terminated,
        counts int32 [n,33,8,4])"""
        n = self.pending() if max_rows is None else min(self.pending(), int(max_rows))
        centres = np.empty(n, dtype=np.int64)
        seqs = np.zeros((n, 34), dtype=np.uint8)
        counts = np.empty((n, 33, 8, 4), dtype=np.int32)
        taken = ctypes.c_int64(0)
        if n:
            self._lib.clair_host_pileup_take(self._h, n, centres.ctypes.data, seqs.ctypes.data, counts.ctypes.data, ctypes.byref(taken))
        return centres, seqs, counts

    def take(self):
        centres, seqs, counts = self.take_arrays()
        return [(int(c), s, counts[i]) for i, (c, s) in enumerate(zip(centres, seqs))]

    def take_text(self, cap=1 << 24):
        """Finished windows as text records (bytes), as many as fit in `cap` bytes; b"" when none is pending."""
        if self._text is None or len(self._text) < cap:
            self._text = ctypes.create_string_buffer(cap)
        n, taken = ctypes.c_int64(0), ctypes.c_int64(0)
        self._lib.clair_host_pileup_take_text(self._h, self.ctg.encode(), self._text, cap, ctypes.byref(n), ctypes.byref(taken))
        return self._text.raw[:n.value]

    def stats(self):
        st = np.zeros(4, dtype=np.int64)
        self._lib.clair_host_pileup_stats(self._h, st.ctypes.data)
        return {"reads": int(st[0]), "open_windows": int(st[1]), "slots_left": int(st[2]), "sorted_path": bool(st[3])}

    def text_from_sam(self, handle, chunk_bytes=1 << 22):
        """Feed a SAM stream (binary or text file object); yield the finished records as text chunks (str)."""
        for _ in feed_stream(self, handle.read, chunk_bytes):
            while self.pending():
                yield self.take_text().decode("latin-1")


class CandidateFinder(_LineSink):
    """clair_host_evc_*: the native twin of clair_amd.extract_variant_candidates.CandidateFinderPy."""

    def __init__(self, ctg_name, reference_sequence, reference_start_0_based, ctg_start=None, ctg_end=None, bed=None,
                 min_coverage=4, threshold=0.125, min_mq=0):
        self._lib = load()
        ref = reference_sequence.encode("latin-1") if isinstance(reference_sequence, str) else bytes(reference_sequence)
        have_range = ctg_start is not None and ctg_end is not None
        if bed is None:
            bs = be = np.zeros(0, dtype=np.int64)
            n_bed = -1
        else:
            bs = np.ascontiguousarray([b[0] for b in bed], dtype=np.int64)
            be = np.ascontiguousarray([b[1] for b in bed], dtype=np.int64)
            n_bed = len(bs)
        out = self._own(self._lib.clair_host_evc_destroy, self._lib.clair_host_last_error)
        self._check(self._lib.clair_host_evc_create(ctg_name.encode(), ref, len(ref), int(reference_start_0_based),
                                                    int(ctg_start) if have_range else -1, int(ctg_end) if have_range else -1,
                                                    bs.ctypes.data, be.ctypes.data, n_bed, float(min_coverage), float(threshold),
                                                    int(min_mq), out), "candidates: ")
        self._feed = self._lib.clair_host_evc_feed
        self._text = None

    @property
    def reads(self):
        return int(self._lib.clair_host_evc_reads(self._h))

    def finish(self):
        self._lib.clair_host_evc_finish(self._h)

    def pending(self):
        return int(self._lib.clair_host_evc_pending(self._h))

    def take_positions(self):
        n = self.pending()
        pos = np.empty(n, dtype=np.int64)
        taken = ctypes.c_int64(0)
        if n:
            self._lib.clair_host_evc_take(self._h, n, pos.ctypes.data, ctypes.byref(taken))
        return pos

    def take_text(self, cap=1 << 22):
        if self._text is None or len(self._text) < cap:
            self._text = ctypes.create_string_buffer(cap)
        n, taken = ctypes.c_int64(0), ctypes.c_int64(0)
        self._lib.clair_host_evc_take_text(self._h, self._text, cap, ctypes.byref(n), ctypes.byref(taken))
        return self._text.raw[:n.value]

    def text_from_sam(self, handle, chunk_bytes=1 << 22):
        for _ in feed_stream(self, handle.read, chunk_bytes):
            while self.pending():
                yield self.take_text().decode("latin-1")


READ_DTYPE = np.dtype([("pos0", "<i8"), ("seq0", "<u4"), ("seq_len", "<u4"), ("op0", "<u4"), ("n_ops", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])
OP_DTYPE = np.dtype([("read", "<u4"), ("code_len", "<u4"), ("ref_off", "<i4"), ("q_off", "<u4")])
READ_REVERSE, READ_EVC, READ_PILE, READ_FLUSH, READ_LOOKUP = 1, 2, 4, 8, 16
# clair_indel_entry_t (include/clair_reads.h): one distinct key of a queried position's indel table; `bases` reads back without its zero padding
ENTRY_DTYPE = np.dtype([("sign", "i1"), ("length", "u1"), ("reserved", "<u2"), ("count", "<u4"), ("first_rank", "<u4"), ("bases", "S50"), ("pad", "u1", (2,))])
LOOKUP_HITS, LOOKUP_ENTRIES = 1, 2          # CLAIR_LOOKUP_*


class SamPacker(_LineSink):
    """clair_host_sampack_*: `samtools view` text -> slabs of packed alignments (include/clair_reads.h) for the device front end."""

    def __init__(self, ctg_name, dcov=250, evc_min_mq=0, pile_min_mq=0, pile_region=None, lookup=False):
        """lookup: pack for the indel look-up too (clair_host_sampack_set_lookup): alignments neither stage walks stay, marked READ_LOOKUP."""
        self._lib = load()
        a, b = (-1, -1) if pile_region is None else (int(pile_region[0]), int(pile_region[1]))
        out = self._own(self._lib.clair_host_sampack_destroy, self._lib.clair_host_last_error)
        self._check(self._lib.clair_host_sampack_create(ctg_name.encode(), int(dcov), int(evc_min_mq), int(pile_min_mq), a, b, out), "sampack: ")
        self._feed = self._lib.clair_host_sampack_feed
        if lookup:
            self._check(self._lib.clair_host_sampack_set_lookup(self._h, 1), "sampack: ")

    def stats(self):
        v = (ctypes.c_int64 * 8)()
        self._lib.clair_host_sampack_stats(self._h, v)
        return dict(zip(("reads", "ops", "elements", "seq_bytes", "anomalies", "lines", "evc_reads", "pile_reads"), [int(x) for x in v]))

    def slab_pointers(self):
        """-> (reads, ops, op_elem, seq) addresses of the slab being filled + its stats; valid until the next feed() / reset()."""
        p = [ctypes.c_void_p() for _ in range(4)]
        self._lib.clair_host_sampack_slab(self._h, *[ctypes.byref(x) for x in p])
        return [x.value or 0 for x in p], self.stats()

    def slab_arrays(self):
        """Copies of the slab as NumPy arrays (tests, the budget replay): reads READ_DTYPE, ops OP_DTYPE, op_elem uint32, seq uint8."""
        (r, o, e, q), st = self.slab_pointers()

        def view(addr, n, dtype):
            if n == 0:
                return np.zeros(0, dtype)
            return np.frombuffer((ctypes.c_char * (n * np.dtype(dtype).itemsize)).from_address(addr), dtype=dtype).copy()
        return view(r, st["reads"], READ_DTYPE), view(o, st["ops"], OP_DTYPE), view(e, st["ops"] + 1, np.uint32), view(q, st["seq_bytes"], np.uint8)

    def reset(self):
        self._lib.clair_host_sampack_reset(self._h)


def indel_table(slabs, positions, capacity=32):
    """clair_host_indel_table: the indel tables of `positions` (1-based, strictly ascending) over slabs = [(reads, ops, op_elem, seq), ...] in
    feed order (SamPacker(lookup=True).slab_arrays()).  -> entries [n][capacity] ENTRY_DTYPE, n_entries, depth (int32), status (uint32)."""
    positions = np.ascontiguousarray(positions, dtype=np.int64)
    n, k = len(positions), len(slabs)
    keep = [(np.ascontiguousarray(s[0], dtype=READ_DTYPE), np.ascontiguousarray(s[1], dtype=OP_DTYPE), np.ascontiguousarray(s[3], dtype=np.uint8)) for s in slabs]
    ptrs = lambda col: (ctypes.c_void_p * max(k, 1))(*[a[col].ctypes.data for a in keep])   # noqa: E731
    sizes = lambda col: (ctypes.c_int64 * max(k, 1))(*[len(a[col]) for a in keep])           # noqa: E731
    entries = np.zeros((n, int(capacity)), dtype=ENTRY_DTYPE)
    n_entries, depth, status = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint32)
    if load().clair_host_indel_table(ptrs(0), sizes(0), ptrs(1), sizes(1), ptrs(2), sizes(2), k, positions.ctypes.data, n, entries.ctypes.data,
                                     int(capacity), n_entries.ctypes.data, depth.ctypes.data, status.ctypes.data) != 0:
        raise ValueError(load().clair_host_last_error().decode())
    return entries, n_entries, depth, status


def tuple_budget_binds(reads, tuples, centres, window_tuples, state):
    """clair_host_tuple_budget_binds over one slab; state = int64[2] carried between slabs ([free slots, first unreleased centre])."""
    reads = np.ascontiguousarray(reads, dtype=READ_DTYPE)
    tuples = np.ascontiguousarray(tuples, dtype=np.uint64)
    centres = np.ascontiguousarray(centres, dtype=np.int64)
    window_tuples = np.ascontiguousarray(window_tuples, dtype=np.uint64)
    binds = ctypes.c_int(0)
    if load().clair_host_tuple_budget_binds(reads.ctypes.data, tuples.ctypes.data, len(reads), centres.ctypes.data, window_tuples.ctypes.data,
                                            len(centres), state.ctypes.data, ctypes.byref(binds)) != 0:
        raise ValueError(load().clair_host_last_error().decode())
    return bool(binds.value)


INFLATE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p)    # clair_host_inflate_fn
INFLATE_BATCH = 2048       # BGZF blocks per device batch (BamReader(inflate="device")): 128 MiB of staging each way
INFLATE_STATUS = ("ok", "corrupt deflate data", "inflated size differs from ISIZE", "CRC32 mismatch")


def inflate_block(data, cap):
    """clair_host_inflate_block: one raw deflate stream through the host twin of the device decoder -> (status, bytes, crc32)."""
    lib = load()
    src = np.frombuffer(bytes(data), dtype=np.uint8) if len(data) else np.zeros(1, dtype=np.uint8)
    out = np.zeros(max(1, int(cap)), dtype=np.uint8)
    n, crc, status = ctypes.c_int64(0), ctypes.c_uint32(0), ctypes.c_int(0)
    if lib.clair_host_inflate_block(src.ctypes.data, len(data), out.ctypes.data, int(cap), ctypes.byref(n), ctypes.byref(crc), ctypes.byref(status)) != 0:
        raise ValueError(lib.clair_host_last_error().decode())
    return int(status.value), out[:n.value].tobytes(), int(crc.value)


def inflate_bgzf(block):
    """clair_host_inflate_bgzf: one whole BGZF block as the device kernel treats it -> (status, bytes)."""
    lib = load()
    src = np.frombuffer(bytes(block), dtype=np.uint8)
    out = np.zeros(65537, dtype=np.uint8)
    n, status = ctypes.c_int64(0), ctypes.c_int(0)
    if lib.clair_host_inflate_bgzf(src.ctypes.data, len(src), out.ctypes.data, ctypes.byref(n), ctypes.byref(status)) != 0:
        raise ValueError(lib.clair_host_last_error().decode())
    return int(status.value), out[:n.value].tobytes()


DEFLATE_MAX_IN = 65280     # bgzip's payload per block (0xff00)


def deflate_bgzf(data):
    """clair_host_deflate_bgzf: at most DEFLATE_MAX_IN bytes -> one whole BGZF block (bytes), the bytes the device compressor writes
    (clair_amd._capi.Deflater).  The call releases the GIL: a thread pool runs blocks side by side."""
    lib = load()
    data = bytes(data)
    out = ctypes.create_string_buffer(65536)
    n = ctypes.c_int64(0)
    if lib.clair_host_deflate_bgzf(ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p), len(data), out, ctypes.byref(n)) != 0:
        raise ValueError(lib.clair_host_last_error().decode())
    return out.raw[:n.value]


class BamError(ValueError):
    """The BAM, its index or the request cannot be read natively (callVarBam turns it into a message and a non-zero exit)."""


def bam_index_for(bam_fn):
    """-> (kind, path) of the index samtools would open for bam_fn: ("bai", <bam>.bai or <stem>.bai), ("csi", <bam>.csi), or (None, None)."""
    stem = bam_fn[:-4] if bam_fn.endswith(".bam") else None
    for path in [bam_fn + ".bai"] + ([stem + ".bai"] if stem else []):
        if os.path.isfile(path):
            return "bai", path
    if os.path.isfile(bam_fn + ".csi") or (stem and os.path.isfile(stem + ".csi")):
        return "csi", bam_fn + ".csi"
    return None, None


class BamReader(Handle):
    """clair_host_bam_*: the records of one contig / region of a BAM, read without samtools (callVarBam --bam_reader native).

        r = BamReader(path, threads=4)                   # inflate="device", device=0: BGZF blocks inflated on the GPU (callVarBam --bam_inflate)
        r.query("chr1", 1000, 2000)                      # 1-based inclusive; None, None = the whole contig
        n_bytes, n_records = r.readinto(buf, offsets)    # whole records, offsets[k] = where record k starts; 0, 0 at the end
        text = r.render(buf, offsets, n_records)         # what `samtools view -F 2316 <bam> <region>` prints for them (11 columns)

    The records readinto() hands out are all those the index yields for the region; the view filter is the consumer's (the device's
    clair_frontend_add_bam or render())."""
    _error = BamError
    _inflater = None

    def __init__(self, path, threads=4, inflate="host", device=0):
        self._lib = load()
        if not 1 <= int(threads) <= 16:
            raise BamError("--bam_threads %d: 1 .. 16" % threads)
        if inflate not in ("host", "device"):
            raise BamError("--bam_inflate %s: host or device" % inflate)
        out = self._own(self._lib.clair_host_bam_close, self._lib.clair_host_last_error)
        self._check(self._lib.clair_host_bam_open(path.encode(), int(threads), out))
        self.path = path
        self.tid, self.region, self.used_index = -1, (-1, -1), False
        self._inflater = self._hook = None
        if inflate == "device":                  # only a function pointer and its context pass between the two libraries
            from clair_amd import _capi
            try:
                self._inflater = _capi.Inflater(device=device, max_blocks=INFLATE_BATCH)
            except _capi.EngineError as e:
                self.close()
                raise BamError(str(e))
            self.set_inflater(self._inflater.callback, self._inflater.handle, INFLATE_BATCH)

    def set_inflater(self, fn, ctx=None, batch_blocks=INFLATE_BATCH):
        """clair_host_bam_set_inflater: fn is a function pointer (an INFLATE_FN instance or an address), None = zlib again."""
        self._hook = fn                          # keeps a Python callback alive
        self._check(self._lib.clair_host_bam_set_inflater(self._h, ctypes.cast(fn, ctypes.c_void_p) if fn is not None else None, ctx, int(batch_blocks)))

    def set_subsample(self, seed, frac):
        """clair_host_bam_set_subsample: render() also drops what `samtools view -s` would (docs/subsample.md); frac <= 0: off."""
        self._check(self._lib.clair_host_bam_set_subsample(self._h, int(seed), float(frac)))

    def close(self):
        Handle.close(self)
        if self._inflater:
            self._inflater.close()
            self._inflater = None

    def info(self):
        v = (ctypes.c_int64 * 4)()
        self._lib.clair_host_bam_info(self._h, v)
        return dict(zip(("n_ref", "eof_block", "records", "used_index"), [int(x) for x in v]))

    def references(self):
        out = []
        for tid in range(self.info()["n_ref"]):
            name, length = ctypes.c_char_p(), ctypes.c_int64(0)
            self._lib.clair_host_bam_ref(self._h, tid, ctypes.byref(name), ctypes.byref(length))
            out.append((name.value.decode(), int(length.value)))
        return out

    def query(self, ctg_name, beg1=None, end1=None, use_index=True):
        """Select ctg_name:beg1-end1 (or the whole contig).  With use_index, the .bai next to the BAM when there is one (a .csi alone is a
        BamError: samtools reads those); without one the records are scanned from the first.  -> True when an index is used."""
        tid = self._lib.clair_host_bam_tid(self._h, ctg_name.encode())
        if tid < 0:
            raise BamError("contig %s is not in the header of %s" % (ctg_name, self.path))
        index = None
        if use_index:
            kind, index = bam_index_for(self.path)
            if kind == "csi":
                raise BamError("%s has only a .csi index, which the native reader does not read: use --bam_reader samtools" % self.path)
        self.tid = tid
        self.region = (-1, -1) if beg1 is None or end1 is None else (int(beg1), int(end1))
        self._check(self._lib.clair_host_bam_query(self._h, None if index is None else index.encode(), tid, self.region[0], self.region[1]))
        self.used_index = index is not None
        return self.used_index

    def readinto(self, buf, offsets, cap=None):
        """Whole records into buf (a writable uint8 array: NumPy, or a page-locked buffer), their starts into offsets (int64 array) ->
        (bytes, records); (0, 0) when the query is exhausted."""
        cap = len(buf) if cap is None else int(cap)
        n_bytes, n_rec = ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self._lib.clair_host_bam_next(self._h, buf.ctypes.data, cap, offsets.ctypes.data, len(offsets), ctypes.byref(n_bytes), ctypes.byref(n_rec)))
        return int(n_bytes.value), int(n_rec.value)

    def voffset(self, k):
        """BGZF virtual offset of record k of the last chunk readinto() handed out."""
        v = ctypes.c_uint64(0)
        self._check(self._lib.clair_host_bam_voffset(self._h, int(k), ctypes.byref(v)))
        return int(v.value)

    def render(self, buf, offsets, n_records):
        """The lines `samtools view -F 2316` prints for those of the n_records records that are on the queried contig and overlap the region."""
        text, n = ctypes.c_void_p(), ctypes.c_int64(0)
        self._check(self._lib.clair_host_bam_render(self._h, buf.ctypes.data, offsets.ctypes.data, int(n_records), self.tid, self.region[0], self.region[1],
                                                    ctypes.byref(text), ctypes.byref(n)))
        return ctypes.string_at(text.value, n.value) if n.value else b""


def subsample_keeps(name, seed, frac):
    """clair_host_subsample_keeps: the subsampling rule for one read name (bytes; it ends at a NUL) -> True when a record of that name stays."""
    name = bytes(name)
    src = np.frombuffer(name + b"\0", dtype=np.uint8)
    rc = load().clair_host_subsample_keeps(src.ctypes.data, len(name), int(seed), float(frac))
    if rc < 0:
        raise ValueError(load().clair_host_last_error().decode())
    return rc == 1


BAM_CHUNK = 64 << 20       # bytes of whole records per BamReader.readinto (the page-locked buffer the device front end reads them from)


def bam_offsets_for(cap):
    """An offsets array for a chunk of cap bytes: a record is at least 36 bytes."""
    return np.empty(max(1, cap // 36 + 1), dtype=np.int64)


class BamText(object):
    """The text `samtools view -F 2316 <bam> <region>` prints, rendered from a BamReader query: read() / readinto() / abort() / finish() like the
    pipe it replaces (callVarBam's host stages and the device front end's host packer)."""

    def __init__(self, reader, chunk=8 << 20):
        self.reader, self.buf, self.offsets = reader, np.empty(chunk, dtype=np.uint8), bam_offsets_for(chunk)
        self.text, self.at, self.eof = b"", 0, False

    def _more(self):
        while not self.eof and self.at >= len(self.text):
            n_bytes, n_rec = self.reader.readinto(self.buf, self.offsets)
            if n_rec == 0:
                self.eof = True
                break
            self.text, self.at = self.reader.render(self.buf, self.offsets, n_rec), 0

    def read(self, n):
        self._more()
        out = self.text[self.at:self.at + n]
        self.at += len(out)
        return out

    def readinto(self, mv):
        piece = self.read(len(mv))
        mv[:len(piece)] = piece
        return len(piece)

    def abort(self):
        self.reader.close()

    def finish(self):
        self.reader.close()
        return 0


def faidx(ref_fn, ctg_name, beg1=None, end1=None):
    """`samtools faidx ref_fn ctg:beg1-end1` (clamped; None = whole contig) without samtools: the bases as str, case kept, or None when the contig
    is not in the .fai (samtools fails there too)."""
    lib = load()
    a, b = (-1, -1) if beg1 is None or end1 is None else (int(beg1), int(end1))
    n = ctypes.c_int64(0)
    if lib.clair_host_faidx(ref_fn.encode(), ctg_name.encode(), a, b, None, 0, ctypes.byref(n)) != 0:
        return None
    out = ctypes.create_string_buffer(max(1, n.value))
    if lib.clair_host_faidx(ref_fn.encode(), ctg_name.encode(), a, b, out, n.value, ctypes.byref(n)) != 0:
        return None
    return out.raw[:n.value].decode("latin-1")


def ensemble_average(probs):
    """clair_host_ensemble_average: probs float32 [K, ...] (K = 1 .. 8 models, in summation order) -> their average [...] float32 as the
    reference's text chain gives it (six decimals out of every model, double sum, six decimals of the mean; docs/ensemble.md).  The CPU
    twin of the device averaging (clair_amd._capi.Engine.ensemble_average, submit_ensemble)."""
    p = np.ascontiguousarray(probs, dtype=np.float32)
    if p.ndim < 1 or p.shape[0] < 1:
        raise ValueError("ensemble_average: probs must be [K, ...] with K >= 1, got %r" % (p.shape,))
    out = np.empty(p.shape[1:], dtype=np.float32)
    if load().clair_host_ensemble_average(p.ctypes.data, p.shape[0], out.size, out.ctypes.data) != 0:
        raise ValueError(load().clair_host_last_error().decode())
    return out


def ensemble_quantise(p):
    """clair_host_ensemble_quantise: the millionths '{:0.6f}'.format(v) prints for each float32 v, as int32."""
    p = np.ascontiguousarray(p, dtype=np.float32)
    out = np.empty(p.shape, dtype=np.int32)
    if load().clair_host_ensemble_quantise(p.ctypes.data, p.size, out.ctypes.data) != 0:
        raise ValueError(load().clair_host_last_error().decode())
    return out


def ensemble_value(millionths):
    """clair_host_ensemble_value: float32 of the six-decimal text of m millionths (0 .. 10^6)."""
    m = np.ascontiguousarray(millionths, dtype=np.int32)
    out = np.empty(m.shape, dtype=np.float32)
    if load().clair_host_ensemble_value(m.ctypes.data, m.size, out.ctypes.data) != 0:
        raise ValueError(load().clair_host_last_error().decode())
    return out


SITE_ORDERS = ("chain", "position")                          # CLAIR_SITES_ORDER_CHAIN, CLAIR_SITES_ORDER_POSITION (include/clair_amd.h)


def site_rows_arguments(n, probs, x, centre, seq):
    """What the add_rows of either site table takes for n candidates -> (probs [n,90], x [n,1056] or None, centre [n,2] or None, seq [n,33] or
    None), contiguous; seq may be uint8 [n,33] / [n,34] (NUL-padded) or a list of str."""
    p = np.ascontiguousarray(probs, dtype=np.float32)
    if p.shape != (n, 90):
        raise ValueError("probs must be float32 [%d,90], got %r" % (n, p.shape))
    if x is not None:
        x = np.ascontiguousarray(x, dtype=np.float32).reshape(len(x), -1)
        if x.shape != (n, N_VALUES):
            raise ValueError("x must hold %d windows of 1056 floats, got %r" % (n, x.shape))
    if centre is not None:
        centre = np.ascontiguousarray(centre, dtype=np.uint8)
        if centre.shape != (n, 2):
            raise ValueError("centre must be uint8 [%d,2], got %r" % (n, centre.shape))
    if seq is not None:
        seq = site_seq_bytes(seq)
        if seq.shape != (n, 33):
            raise ValueError("seq must hold %d reference windows, got %r" % (n, seq.shape))
    return p, x, centre, seq


def site_seq_bytes(seq):
    """Reference windows as the site tables keep them: uint8 [n,33], NUL-padded (from [n,33], [n,34] or a list of str)."""
    if isinstance(seq, np.ndarray) and seq.dtype == np.uint8 and seq.ndim == 2 and seq.shape[1] in (33, 34):
        return np.ascontiguousarray(seq[:, :33])
    out = np.zeros((len(seq), 33), dtype=np.uint8)
    for i, text in enumerate(seq):
        raw = (text.encode("latin-1") if isinstance(text, str) else bytes(text))[:33]
        out[i, :len(raw)] = np.frombuffer(raw, dtype=np.uint8)
    return out


class HostSiteTable(Handle):
    """clair_host_sites_*: the site table of ensemble calling across BAMs on the CPU, the twin of clair_amd._capi.SiteTable (same methods, same
    bits).

        t = HostSiteTable()
        for each source:  t.begin_source(positions);  for each run:  t.add_rows(first, probs, x, centre, seq)
        n_out = t.finish(min_count, "chain");  t.info(0, n_out), t.rows(0, n_out), t.windows(0, n_out)"""

    def __init__(self):
        self._lib = load()
        out = self._own(self._lib.clair_host_sites_destroy, self._lib.clair_host_last_error)
        self._check(self._lib.clair_host_sites_create(out))
        self.n_out = 0

    def begin_source(self, positions):
        """-> how many of the positions (int64, strictly ascending) the table did not have"""
        p = np.ascontiguousarray(positions, dtype=np.int64)
        n_new = i64(0)
        self._check(self._lib.clair_host_sites_begin_source(self._h, p.ctypes.data, len(p), ctypes.byref(n_new)))
        return int(n_new.value)

    def add_rows(self, first, probs, x=None, centre=None, seq=None):
        n = len(probs)
        p, x, centre, seq = site_rows_arguments(n, probs, x, centre, seq)
        self._check(self._lib.clair_host_sites_add_rows(self._h, int(first), p.ctypes.data, n, *[a.ctypes.data if a is not None else None for a in (x, centre, seq)]))

    def finish(self, min_count=0, order="chain"):
        n_out = i64(0)
        self._check(self._lib.clair_host_sites_finish(self._h, int(min_count), SITE_ORDERS.index(order), ctypes.byref(n_out)))
        self.n_out = int(n_out.value)
        return self.n_out

    def info(self, first, n):
        """-> (positions int64 [n], counts int32 [n], seq uint8 [n,34] NUL-terminated) of entries [first, first + n) of the output list"""
        positions, counts, seq = np.empty(n, np.int64), np.empty(n, np.int32), np.zeros((n, 33), np.uint8)
        self._check(self._lib.clair_host_sites_info(self._h, int(first), int(n), positions.ctypes.data, counts.ctypes.data, seq.ctypes.data))
        return positions, counts, np.concatenate([seq, np.zeros((n, 1), np.uint8)], axis=1)

    def rows(self, first, n):
        out = np.empty((n, 90), dtype=np.float32)
        self._check(self._lib.clair_host_sites_rows(self._h, int(first), int(n), out.ctypes.data))
        return out

    def windows(self, first, n):
        x = np.empty((n, 33, 8, 4), dtype=np.float32)
        self._check(self._lib.clair_host_sites_windows(self._h, int(first), int(n), x.ctypes.data))
        return x


# clair_overlap_span (clair_amd/csrc/overlap_core.h): one VCF row as the overlap filter sees it; flags bit 0 = OVERLAP_SNP
SPAN_DTYPE = np.dtype([("pos", "<i8"), ("ctg", "<i4"), ("qual", "<i4"), ("del", "<i4"), ("flags", "<u4")])
assert SPAN_DTYPE.itemsize == 24
OVERLAP_SNP = 1


def overlap_keep(spans):
    """clair_host_overlap_keep: spans (SPAN_DTYPE [n], input order) -> uint8 [n], 1 for the rows the overlap filter prints.  The CPU twin of
    clair_amd._capi.overlap_keep."""
    s = np.ascontiguousarray(spans, dtype=SPAN_DTYPE)
    keep = np.zeros(len(s), dtype=np.uint8)
    if load().clair_host_overlap_keep(s.ctypes.data, len(s), keep.ctypes.data) != 0:
        raise ValueError(load().clair_host_last_error().decode())
    return keep


# ---- the training-set builder's rules over arrays (clair_host_train_set_*, csrc/train_set_core.h): the CPU twin of _capi.Frontend.sample_candidates / .pair
TS_OUTSIDE, TS_NEAR, TS_TRUTH = 0, 1, 2
TS_STAGE_SAMPLE, TS_STAGE_PAIR = 1, 2


def _ts_check(rc):
    if rc != 0:
        raise ValueError(load().clair_host_last_error().decode())


def merged_bed(bed):
    """[(start, end), ...] of one contig or None -> (starts int64, ends int64, n or -1): sorted, empty intervals widened by one, merged
    (extract_variant_candidates.BedRegions, shared/interval_tree.py)."""
    if bed is None:
        z = np.zeros(0, dtype=np.int64)
        return z, z, -1
    from .extract_variant_candidates import BedRegions
    r = BedRegions(bed)
    return np.array(r.start, dtype=np.int64), np.array(r.end, dtype=np.int64), len(r.start)


def train_set_key(ctg_name, seed, stage):
    """key(seed, ctg, stage) as a signed 64-bit integer (the bits are what counts)."""
    key = ctypes.c_int64(0)
    _ts_check(load().clair_host_train_set_key(ctg_name.encode(), ctypes.c_int64(int(seed) & (2 ** 64 - 1)).value, int(stage), ctypes.byref(key)))
    return key.value


def train_set_sample(positions, truth, p_near, p_outside, key):
    """-> (class uint8 [n], draw uint64 [n], sampled uint8 [n], n_near, n_outside) of 1-based positions against ascending truth positions."""
    p = np.ascontiguousarray(positions, dtype=np.int64)
    t = np.ascontiguousarray(truth, dtype=np.int64)
    cls, draws, sampled = np.zeros(len(p), np.uint8), np.zeros(len(p), np.uint64), np.zeros(len(p), np.uint8)
    near, outside = ctypes.c_int64(0), ctypes.c_int64(0)
    _ts_check(load().clair_host_train_set_sample(p.ctypes.data, len(p), t.ctypes.data, len(t), float(p_near), float(p_outside), int(key), cls.ctypes.data,
                                                 draws.ctypes.data, sampled.ctypes.data, ctypes.byref(near), ctypes.byref(outside)))
    return cls, draws, sampled, near.value, outside.value


def train_set_pair_count(centres, truth, bed):
    """-> (v, c): windows at a truth position, usable non-variant windows (bed: intervals of the contig or None)."""
    p = np.ascontiguousarray(centres, dtype=np.int64)
    t = np.ascontiguousarray(truth, dtype=np.int64)
    bs, be, nb = merged_bed(bed)
    v, c = ctypes.c_int64(0), ctypes.c_int64(0)
    _ts_check(load().clair_host_train_set_pair_count(p.ctypes.data, len(p), t.ctypes.data, len(t), bs.ctypes.data, be.ctypes.data, nb, ctypes.byref(v), ctypes.byref(c)))
    return v.value, c.value


def train_set_ratio(v, amp, c):
    r = f64(0)
    _ts_check(load().clair_host_train_set_ratio(int(v), float(amp), int(c), ctypes.byref(r)))
    return r.value


def train_set_pair_keep(centres, truth, bed, r, key):
    """-> (indices int64 of the kept windows: variant ones first, each part in input order; how many of them are variant windows)"""
    p = np.ascontiguousarray(centres, dtype=np.int64)
    t = np.ascontiguousarray(truth, dtype=np.int64)
    bs, be, nb = merged_bed(bed)
    kept = np.zeros(max(len(p), 1), dtype=np.int64)
    kv, kn = ctypes.c_int64(0), ctypes.c_int64(0)
    _ts_check(load().clair_host_train_set_pair_keep(p.ctypes.data, len(p), t.ctypes.data, len(t), bs.ctypes.data, be.ctypes.data, nb, float(r), int(key),
                                                    kept.ctypes.data, ctypes.byref(kv), ctypes.byref(kn)))
    return kept[:kv.value + kn.value], kv.value


def train_set_pair(centres, truth, bed, amp, key):
    """The pairing of one contig's windows -> (kept indices, stats dict v, c, r, kept_var, kept_non)."""
    v, c = train_set_pair_count(centres, truth, bed)
    r = train_set_ratio(v, amp, c)
    kept, kv = train_set_pair_keep(centres, truth, bed, r, key)
    return kept, dict(v=v, c=c, r=r, kept_var=kv, kept_non=len(kept) - kv)


def train_set_labels(centres, centre_base, truth, truth_labels, bed):
    """-> (labels uint8 [n,4], in_set uint8 [n]); centre_base uint8 [n] = refseq[16] of each window, truth_labels uint8 [n_truth,4]."""
    p = np.ascontiguousarray(centres, dtype=np.int64)
    b = np.ascontiguousarray(centre_base, dtype=np.uint8)
    t = np.ascontiguousarray(truth, dtype=np.int64)
    tl = np.ascontiguousarray(truth_labels, dtype=np.uint8).reshape(len(t), 4)
    bs, be, nb = merged_bed(bed)
    labels, in_set = np.zeros((len(p), 4), np.uint8), np.zeros(len(p), np.uint8)
    _ts_check(load().clair_host_train_set_labels(p.ctypes.data, b.ctypes.data, len(p), t.ctypes.data, tl.ctypes.data, len(t), bs.ctypes.data, be.ctypes.data, nb,
                                                 labels.ctypes.data, in_set.ctypes.data))
    return labels, in_set
