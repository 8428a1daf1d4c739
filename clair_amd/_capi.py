"""ctypes binding of the C ABI in include/clair_amd.h (libclair_amd.so, built by build.py).

There is deliberately no fallback: if the shared library is missing or no HIP device is
present, construction of an engine raises.  The HIP path is the product.
"""
import ctypes
import os

import numpy as np

from clair_amd._hostapi import INFLATE_STATUS, Handle

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CLAIR_AMD_LIB") or os.path.join(_HERE, "libclair_amd.so")   # override: debugging builds only

c_int, c_i64, c_vp, c_cp, c_dbl = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_double
p_vp, p_i64 = ctypes.POINTER(c_vp), ctypes.POINTER(c_i64)


def _sig(*argtypes, **kw):
    """One row of SIGNATURES: (restype, argtypes); a function returns int unless restype= says otherwise."""
    return kw.get("restype", c_int), list(argtypes)


_SUBMIT_EX = (c_vp, c_int, c_vp, c_int, c_i64, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp)
_INFLATE_BLOCKS = (c_vp, c_vp, c_i64, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp)
# every function include/clair_amd.h declares, with its prototype there as ctypes states it (tests/test_abi.py checks header <-> this table <-> .so):
# the one place to add an entry point
SIGNATURES = {
    "clair_abi_version": _sig(),
    "clair_device_count": _sig(),
    "clair_device_pci_bus_id": _sig(c_int, c_cp, c_int),
    "clair_last_error": _sig(c_vp, restype=c_cp),
    "clair_engine_create": _sig(c_int, c_int, c_int, p_vp),
    "clair_engine_destroy": _sig(c_vp, restype=None),
    "clair_set_tensor": _sig(c_vp, c_int, c_vp, c_i64),
    "clair_finalize_weights": _sig(c_vp),
    "clair_predict": _sig(c_vp, c_vp, c_int, c_vp, c_vp, c_vp, c_vp),
    "clair_submit": _sig(c_vp, c_int, c_vp, c_int, c_vp, c_vp, c_vp, c_vp),
    "clair_wait": _sig(c_vp, c_int),
    "clair_slot_input": _sig(c_vp, c_int, p_vp),
    "clair_submit_counts": _sig(c_vp, c_int, c_vp, c_int, c_vp, c_vp, c_vp, c_vp),
    "clair_submit_ex": _sig(*_SUBMIT_EX),
    "clair_decode": _sig(c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_vp),
    "clair_pinned_alloc": _sig(c_vp, c_i64, p_vp),
    "clair_pinned_free": _sig(c_vp, c_vp),
    "clair_eval_reset": _sig(c_vp),
    "clair_submit_eval": _sig(c_vp, c_int, c_vp, c_int, c_i64, c_int, c_vp, c_vp, c_vp, c_vp, c_vp),
    "clair_eval": _sig(c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_int),
    "clair_eval_read": _sig(c_vp, c_vp),
    "clair_ensemble_models": _sig(c_vp, c_int),
    "clair_ensemble_set_tensor": _sig(c_vp, c_int, c_int, c_vp, c_i64),
    "clair_ensemble_finalize_weights": _sig(c_vp, c_int),
    "clair_submit_ensemble": _sig(*_SUBMIT_EX),
    "clair_ensemble_average": _sig(c_vp, c_int, c_vp, c_int, c_int, c_vp),
    "clair_sites_create": _sig(c_vp, p_vp),
    "clair_sites_destroy": _sig(c_vp, restype=None),
    "clair_sites_begin_source": _sig(c_vp, c_vp, c_i64, p_i64),
    "clair_submit_sites": _sig(c_vp, c_int, c_vp, c_i64, c_vp, c_int, c_i64, c_int, c_vp, c_vp),
    "clair_sites_add_rows": _sig(c_vp, c_vp, c_i64, c_vp, c_int, c_vp, c_vp, c_vp),
    "clair_sites_finish": _sig(c_vp, c_int, c_int, p_i64),
    "clair_sites_info": _sig(c_vp, c_i64, c_i64, c_vp, c_vp, c_vp),
    "clair_sites_rows": _sig(c_vp, c_i64, c_i64, c_vp),
    "clair_sites_windows": _sig(c_vp, c_i64, c_i64, c_vp),
    "clair_submit_site_calls": _sig(c_vp, c_int, c_vp, c_i64, c_int, c_vp, c_vp, c_vp, c_vp, c_vp),
    "clair_dataset_alloc": _sig(c_vp, c_i64, p_vp, p_vp),
    "clair_dataset_free": _sig(c_vp, c_vp, c_vp),
    "clair_dataset_upload": _sig(c_vp, c_vp, c_i64, c_vp, c_i64),
    "clair_dataset_download": _sig(c_vp, c_vp, c_i64, c_vp, c_i64),
    "clair_run_resident": _sig(c_vp, c_int, c_vp, c_vp, c_i64, c_int),
    "clair_sync": _sig(c_vp),
    "clair_timing_enable": _sig(c_vp, c_int),
    "clair_kernel_times": _sig(c_vp, c_vp, c_vp),
    "clair_timing_reset": _sig(c_vp),
    "clair_kernel_workgroups": _sig(c_vp, c_int, c_vp),
    "clair_engine_counter": _sig(c_vp, c_int, p_i64),
    "clair_debug_read": _sig(c_vp, c_int, c_int, c_vp, c_i64),
    "clair_comm_preflight": _sig(c_int),
    "clair_comm_unique_id": _sig(c_vp),
    "clair_comm_create": _sig(c_int, c_int, c_int, c_vp, p_vp),
    "clair_comm_create_timed": _sig(c_int, c_int, c_int, c_vp, c_int, p_vp),
    "clair_comm_destroy": _sig(c_vp, restype=None),
    "clair_comm_abort": _sig(c_vp, restype=None),
    "clair_comm_last_error": _sig(c_vp, restype=c_cp),
    "clair_comm_barrier": _sig(c_vp),
    "clair_comm_allreduce_f64": _sig(c_vp, c_vp, c_int, c_int),
    "clair_comm_broadcast": _sig(c_vp, c_vp, c_i64, c_int),
    "clair_comm_allgather": _sig(c_vp, c_vp, c_vp, c_i64),
    "clair_comm_allgather_device": _sig(c_vp, c_vp, c_vp, c_i64),
    "clair_frontend_create": _sig(c_int, c_cp, c_i64, c_i64, c_i64, c_i64, p_vp),
    "clair_frontend_destroy": _sig(c_vp, restype=None),
    "clair_frontend_last_error": _sig(c_vp, restype=c_cp),
    "clair_frontend_add_reads": _sig(c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_i64),
    "clair_frontend_text_options": _sig(c_vp, c_cp, c_int, c_int, c_int, c_i64, c_i64),
    "clair_frontend_add_text": _sig(c_vp, c_vp, c_i64),
    "clair_frontend_text_stats": _sig(c_vp, c_vp),
    "clair_frontend_slab_reads": _sig(c_vp, c_i64, c_vp, c_i64, p_i64),
    "clair_frontend_bam_options": _sig(c_vp, c_int, c_int, c_int, c_int, c_i64, c_i64, c_i64, c_i64),
    "clair_frontend_add_bam": _sig(c_vp, c_vp, c_i64, c_vp, c_i64),
    "clair_frontend_bam_lookup": _sig(c_vp, c_int),
    "clair_frontend_bam_subsample": _sig(c_vp, c_i64, c_dbl),
    "clair_frontend_indel_table": _sig(c_vp, c_vp, c_i64, c_vp, c_int, c_vp, c_vp, c_vp),
    "clair_frontend_find_candidates": _sig(c_vp, c_dbl, c_dbl, c_i64, c_i64, c_vp, c_vp, c_i64, p_i64),
    "clair_frontend_set_candidates": _sig(c_vp, c_vp, c_i64, p_i64),
    "clair_frontend_get_candidates": _sig(c_vp, c_vp),
    "clair_frontend_build_windows": _sig(c_vp, c_int, c_int, p_i64),
    "clair_frontend_build_windows_ex": _sig(c_vp, c_int, c_int, c_int, p_i64),
    "clair_frontend_window_info": _sig(c_vp, c_i64, c_i64, c_vp, c_vp),
    "clair_frontend_window_counts": _sig(c_vp, c_i64, c_i64, c_vp),
    "clair_frontend_counts_device": _sig(c_vp, c_i64, restype=c_vp),
    "clair_frontend_sample_candidates": _sig(c_vp, c_dbl, c_i64, c_i64, c_vp, c_vp, c_i64, c_vp, c_i64, c_dbl, c_dbl, c_i64, c_int, p_i64, p_i64, p_i64),
    "clair_frontend_pair": _sig(c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_dbl, c_i64, c_vp),
    "clair_frontend_train_set_info": _sig(c_vp, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp),
    "clair_frontend_train_set_counts": _sig(c_vp, c_i64, c_i64, c_vp),
    "clair_frontend_budget_inputs": _sig(c_vp, c_i64, c_vp, c_vp, c_vp),
    "clair_frontend_stats": _sig(c_vp, c_vp),
    "clair_frontend_position_tallies": _sig(c_vp, c_i64, c_i64, c_vp),
    "clair_frontend_gvcf_blocks": _sig(c_vp, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, p_i64),
    "clair_frontend_gvcf_device_ms": _sig(c_vp, c_vp),
    "clair_inflate_create": _sig(c_int, c_int, p_vp),
    "clair_inflate_destroy": _sig(c_vp, restype=None),
    "clair_inflate_last_error": _sig(c_vp, restype=c_cp),
    "clair_inflate_blocks": _sig(*_INFLATE_BLOCKS),
    "clair_inflate_blocks_cb": _sig(*_INFLATE_BLOCKS),
    "clair_deflate_create": _sig(c_int, c_int, p_vp),
    "clair_deflate_destroy": _sig(c_vp, restype=None),
    "clair_deflate_last_error": _sig(c_vp, restype=c_cp),
    "clair_deflate_blocks": _sig(c_vp, c_vp, c_i64, c_int, c_vp, c_vp, c_vp, c_vp),
    "clair_overlap_keep": _sig(c_int, c_vp, c_i64, c_vp),
    "clair_overlap_last_error": _sig(restype=c_cp),
    "clair_compare_create": _sig(c_int, p_vp),
    "clair_compare_destroy": _sig(c_vp, restype=None),
    "clair_compare_last_error": _sig(c_vp, restype=c_cp),
    "clair_compare_set_contigs": _sig(c_vp, c_vp, c_vp, c_int),
    "clair_compare_set_regions": _sig(c_vp, c_vp, c_vp, c_vp, c_i64),
    "clair_compare_parse": _sig(c_vp, c_int, c_vp, c_i64, c_vp),
    "clair_compare_keys": _sig(c_vp, c_int, c_vp),
    "clair_compare_permute": _sig(c_vp, c_int, c_vp),
    "clair_compare_run": _sig(c_vp),
    "clair_compare_counts": _sig(c_vp, c_vp),
    "clair_compare_records": _sig(c_vp, c_int, c_vp, c_vp),
    "clair_compare_set_reference": _sig(c_vp, c_vp, c_vp, c_int),
    "clair_compare_left_align": _sig(c_vp, c_int, c_vp),
    "clair_compare_allele_text": _sig(c_vp, c_int, c_vp),
    "clair_train_create": _sig(c_int, c_int, c_int, c_int, p_vp),
    "clair_train_destroy": _sig(c_vp, restype=None),
    "clair_train_last_error": _sig(c_vp, restype=c_cp),
    "clair_train_set_tensor": _sig(c_vp, c_int, c_int, c_vp, c_i64),
    "clair_train_get_tensor": _sig(c_vp, c_int, c_int, c_vp, c_i64),
    "clair_train_config": _sig(c_vp, c_vp, c_vp, c_vp, c_i64),
    "clair_train_zero_grad": _sig(c_vp),
    "clair_train_accumulate": _sig(c_vp, c_vp, c_vp, c_int, c_i64, c_int, c_vp),
    "clair_train_step": _sig(c_vp, c_dbl, c_dbl, c_vp),
    "clair_train_read_mask": _sig(c_vp, c_int, c_vp, c_i64),
    "clair_train_probabilities": _sig(c_vp, c_vp),
    "clair_train_accuracy": _sig(c_vp, c_vp),
    "clair_train_debug_gemm": _sig(c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp),
    "clair_train_debug_column_sum": _sig(c_vp, c_vp, c_i64, c_i64, c_int, c_i64, c_vp, c_i64, c_int, c_int, c_int),
    "clair_bamidx_create": _sig(c_int, c_int, c_int, p_vp),
    "clair_bamidx_destroy": _sig(c_vp, restype=None),
    "clair_bamidx_last_error": _sig(c_vp, restype=c_cp),
    "clair_bamidx_begin": _sig(c_vp, c_int, c_vp),
    "clair_bamidx_batch": _sig(c_vp, c_vp, c_i64, c_int, c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_int, c_vp, p_vp),
    "clair_bamidx_finish": _sig(c_vp, c_vp, c_i64, c_vp),
    "clair_bamidx_backend": _sig(c_vp, c_vp),
    "clair_bamidx_debug_frame": _sig(c_vp, c_vp, c_i64, c_i64, c_vp, c_i64, c_vp),
    "clair_bamsort_create": _sig(c_int, c_int, c_int, p_vp),
    "clair_bamsort_destroy": _sig(c_vp, restype=None),
    "clair_bamsort_last_error": _sig(c_vp, restype=c_cp),
    "clair_bamsort_begin": _sig(c_vp, c_int, c_vp, c_i64),
    "clair_bamsort_pass": _sig(c_vp, c_i64, c_i64, c_int),
    "clair_bamsort_batch": _sig(c_vp, c_vp, c_i64, c_int, c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_int, c_vp),
    "clair_bamsort_histogram": _sig(c_vp, c_vp, c_i64),
    "clair_bamsort_sort": _sig(c_vp, c_int, c_vp),
    "clair_bamsort_emit": _sig(c_vp, c_i64, c_int, c_int, c_vp, c_vp),
    "clair_bamsort_backend": _sig(c_vp, c_vp),
    "clair_bamsort_debug_sort": _sig(c_vp, c_vp, c_i64, c_vp),
    "clair_bamsort_debug_gather": _sig(c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_i64),
    "clair_markdup_create": _sig(c_int, c_int, c_int, p_vp),
    "clair_markdup_destroy": _sig(c_vp, restype=None),
    "clair_markdup_last_error": _sig(c_vp, restype=c_cp),
    "clair_markdup_begin": _sig(c_vp, c_int, c_i64, c_int),
    "clair_markdup_batch": _sig(c_vp, c_vp, c_i64, c_int, c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_int, c_vp),
    "clair_markdup_resolve": _sig(c_vp),
    "clair_markdup_mark": _sig(c_vp, c_vp, c_i64, c_int, c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_int, c_vp),
    "clair_markdup_emit": _sig(c_vp, c_i64, c_int, c_int, c_vp, c_vp),
    "clair_markdup_stats": _sig(c_vp, c_vp),
    "clair_markdup_backend": _sig(c_vp, c_vp),
    "clair_markdup_debug_summary": _sig(c_vp, c_vp, c_i64, c_vp, c_i64, c_int, c_vp),
    "clair_markdup_debug_resolve": _sig(c_vp, c_vp, c_i64, c_vp),
    "clair_markdup_debug_mark": _sig(c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_int, c_vp, c_vp, c_vp),
}
SYMBOLS = tuple(SIGNATURES)
ENSEMBLE_MAX_MODELS = 8                                      # CLAIR_ENSEMBLE_MAX_MODELS
OVERLAP_SCAN_BLOCK = 2048                                    # clair_ov::BLOCK (csrc/overlap.hip): rows per workgroup of the head scan
GVCF_SCAN_TILE = 2048                                        # clair_gv::TILE (csrc/gvcf.hip): positions per workgroup of the block scan
COMPARE_SCAN_BLOCK = 2048                                    # clair_cmp::BLOCK (csrc/compare.hip): text bytes / record slots per workgroup of a scan
EVAL_COUNTS = 3 + 21 * 21 + 3 * 3 + 33 * 33 + 33 * 33      # CLAIR_EVAL_COUNTS: all, top1, top2, gt21, genotype, len1, len2
KERNEL_NAMES = ("proj1", "lstm1", "proj2", "lstm2", "l3", "l4", "tail", "decode")

_lib = None
_libs = {}


class EngineError(RuntimeError):
    pass


def load(path=None):
    """Load libclair_amd.so (CDLL: calls release the GIL, as TF's session.run does for the
    reference's predict thread, clair/call_var.py:1343).  `path` names another BUILD of the same sources (the wait-all check
    build of tools/gpu/waitall_compare.py); it never names a different implementation."""
    global _lib
    if path is None and _lib is not None:
        return _lib
    if path is not None and path in _libs:
        return _libs[path]
    lib_path = path or LIB_PATH
    if not os.path.isfile(lib_path):
        raise EngineError(
            "%s not found: build the HIP extension first (python -m clair_amd.build, or "
            "__graft_entry__.build()). There is no CPU fallback." % lib_path)
    lib = ctypes.CDLL(lib_path)
    # an OLDER build of the same sources, named explicitly (A/B timing, tools/gpu/ab_libs.sh), may predate the newest entry points: those stay unbound
    older_ok = path is not None or bool(os.environ.get("CLAIR_AMD_LIB"))
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name, None) if older_ok else getattr(lib, name)    # AttributeError: this tree's own build lacks a declared entry point
        if fn is None:
            continue
        fn.restype, fn.argtypes = restype, argtypes
    if path is None:
        _lib = lib
    else:
        _libs[path] = lib
    return lib


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def prepare_batch(batch, counts):
    """What clair_submit_ex / clair_submit_eval / clair_submit_ensemble take of a batch -> (keep_alive, address, is_counts, stride_bytes, n).
    batch: [n,33,8,4] float32, or int16 with counts=True -- a strided view whose candidates are dense (the counts column of an array of
    binary tensor records) goes through as it lies, anything else is copied to a contiguous array of the right dtype; or windows already in
    device memory as int16 counts, a DeviceWindows or an (address, n) tuple: the address goes through as it is."""
    if isinstance(batch, DeviceWindows):
        return batch, ctypes.c_void_p(batch.address), 1, 0, len(batch)
    if isinstance(batch, tuple):
        return None, ctypes.c_void_p(int(batch[0])), 1, 0, int(batch[1])
    dtype = np.int16 if counts else np.float32
    x = np.asarray(batch)
    if x.ndim != 4 or x.shape[1:] != (33, 8, 4):
        raise ValueError("batch must have shape [n,33,8,4], got %r" % (x.shape,))
    n = x.shape[0]
    inner_dense = x.dtype == dtype and n > 0 and x[0].flags.c_contiguous and x.strides[0] >= x[0].nbytes
    if not inner_dense:
        x = np.ascontiguousarray(x, dtype=dtype)
    return x, _ptr(x), int(bool(counts)), 0 if x.flags.c_contiguous else int(x.strides[0]), n


class DeviceHandle(Handle):
    """A handle of this library: its last-error function takes the handle (NULL after a failed create), failures are EngineError."""

    def _check(self, rc, what):
        if rc != 0:
            raise EngineError("%s failed: %s" % (what, self._last_error(self._h).decode()))


class Engine(DeviceHandle):
    """Thin object wrapper over one clair_engine_t."""

    def __init__(self, device=0, max_batch=1024, n_slots=1, lib_path=None):
        self._lib = load(lib_path)
        self.max_batch = int(max_batch)
        self.n_slots = int(n_slots)
        out = self._own(self._lib.clair_engine_destroy, self._lib.clair_last_error)
        self._check(self._lib.clair_engine_create(int(device), int(max_batch), int(n_slots), out), "clair_engine_create")
        self._pending = {}
        self.n_models = 1
        self._tables = []                   # weak references to the site tables of this handle: they go before it does

    def close(self):
        for ref in getattr(self, "_tables", []):
            table = ref()
            if table is not None:
                table.close()
        self._tables = []
        DeviceHandle.close(self)

    # -- weights ---------------------------------------------------------------------------
    def load_weights(self, w):
        from clair_amd.weights import TENSOR_IDS, check_weights
        check_weights(w)
        for key, tid in TENSOR_IDS.items():
            a = np.ascontiguousarray(w[key], dtype=np.float32)
            self._check(self._lib.clair_set_tensor(self._h, tid, _ptr(a), a.size), "clair_set_tensor(%s)" % key)
        self._check(self._lib.clair_finalize_weights(self._h), "clair_finalize_weights")

    def load_ensemble(self, list_of_weights):
        """clair_ensemble_*: the checkpoints of an ensemble, 1 .. ENSEMBLE_MAX_MODELS dicts as load_weights takes them.  The first is
        image 0, what predict / submit / submit_calls go on using alone; submit_ensemble runs them all, summed in this order."""
        from clair_amd.weights import TENSOR_IDS, check_weights
        ws = list(list_of_weights)
        if not 1 <= len(ws) <= ENSEMBLE_MAX_MODELS:
            raise ValueError("an ensemble has 1 .. %d checkpoints, got %d" % (ENSEMBLE_MAX_MODELS, len(ws)))
        for w in ws:
            check_weights(w)
        self._check(self._lib.clair_ensemble_models(self._h, len(ws)), "clair_ensemble_models")
        self.n_models = len(ws)
        for model, w in enumerate(ws):
            for key, tid in TENSOR_IDS.items():
                a = np.ascontiguousarray(w[key], dtype=np.float32)
                self._check(self._lib.clair_ensemble_set_tensor(self._h, model, tid, _ptr(a), a.size), "clair_ensemble_set_tensor(%d, %s)" % (model, key))
            self._check(self._lib.clair_ensemble_finalize_weights(self._h, model), "clair_ensemble_finalize_weights(%d)" % model)

    # -- predict ---------------------------------------------------------------------------
    @staticmethod
    def _prep_x(x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim < 2 or x.size != x.shape[0] * 1056:
            raise ValueError("input must be [n,33,8,4] float32, got shape %s" % (x.shape,))
        return x

    @staticmethod
    def _alloc_out(n):
        return [np.empty((n, m), dtype=np.float32) for m in (21, 3, 33, 33)]

    def predict(self, x):
        x = self._prep_x(x)
        outs = self._alloc_out(x.shape[0])
        self._check(self._lib.clair_predict(self._h, _ptr(x), x.shape[0], *[_ptr(o) for o in outs]), "clair_predict")
        return outs

    def submit(self, slot, x):
        x = self._prep_x(x)
        outs = self._alloc_out(x.shape[0])
        self._check(self._lib.clair_submit(self._h, slot, _ptr(x), x.shape[0], *[_ptr(o) for o in outs]), "clair_submit")
        self._pending[slot] = (x, outs)  # keep the buffers alive until wait()

    def submit_counts(self, slot, counts):
        """submit() for raw pileup counts [n,33,8,4] int16 (channel 0 not yet subtracted): half the bytes on the host link,
        conversion on the device; pair with wait(slot)."""
        c = np.ascontiguousarray(counts, dtype=np.int16)
        if c.ndim != 4 or c.shape[1:] != (33, 8, 4):
            raise ValueError("counts must have shape [n,33,8,4], got %r" % (c.shape,))
        outs = self._alloc_out(c.shape[0])
        self._check(self._lib.clair_submit_counts(self._h, slot, _ptr(c), c.shape[0], *[_ptr(o) for o in outs]), "clair_submit_counts")
        self._pending[slot] = (c, outs)

    def submit_calls(self, slot, batch, centre, counts=False, with_probabilities=False):
        """clair_submit_ex: forward pass + decode on the device.  batch: [n,33,8,4] float32, or raw int16 counts with counts=True (the
        candidates may be a strided view, e.g. the counts column of an array of binary tensor records: no copy is made here);
        centre: uint8 [n,2] (clair_amd._hostapi.centre_bytes).  wait(slot) then returns the call records (structured array,
        _hostapi.CALL_DTYPE), or (records, [gt21, genotype, len1, len2]) with with_probabilities=True."""
        self._submit_ex(self._lib.clair_submit_ex, "clair_submit_ex", slot, batch, centre, counts, with_probabilities)

    def submit_ensemble(self, slot, batch, centre=None, counts=False, with_probabilities=False):
        """clair_submit_ensemble: submit_calls with every checkpoint of load_ensemble -- the batch comes in once, the forward passes run
        back to back, their probabilities are averaged on the device as the reference's text chain averages them (docs/ensemble.md)
        and the averaged rows are decoded.  Same arguments and the same results from wait(slot) as submit_calls; centre=None asks for
        no call records: wait(slot) then returns the averaged [gt21, genotype, len1, len2] alone."""
        self._submit_ex(self._lib.clair_submit_ensemble, "clair_submit_ensemble", slot, batch, centre, counts, with_probabilities)

    def _submit_ex(self, fn, what, slot, batch, centre, counts, with_probabilities):
        from clair_amd._hostapi import CALL_DTYPE
        keep, ptr, is_counts, stride, n = prepare_batch(batch, counts)
        c = calls = None
        if centre is not None:
            c = np.ascontiguousarray(centre, dtype=np.uint8)
            if c.shape != (n, 2):
                raise ValueError("centre must be uint8 [%d,2], got %r" % (n, c.shape))
            calls = np.zeros(n, dtype=CALL_DTYPE)
        outs = self._alloc_out(n) if with_probabilities or calls is None else None
        ptrs = [_ptr(o) for o in outs] if outs else [None] * 4
        self._check(fn(self._h, int(slot), ptr, is_counts, stride, n, _ptr(c) if c is not None else None, _ptr(calls) if calls is not None else None, *ptrs), what)
        self._pending[slot] = ((keep, c), outs if calls is None else ((calls, outs) if outs else calls))

    def ensemble_average(self, probs, slot=0):
        """clair_ensemble_average: the device averaging alone.  probs: float32 [K, n, 90] packed rows of K models (or a list of K
        [gt21, genotype, len1, len2] lists) -> the averaged rows [n, 90] (split_outputs gives the four arrays)."""
        if isinstance(probs, (list, tuple)) and len(probs) and isinstance(probs[0], (list, tuple)):
            probs = np.stack([np.concatenate([np.asarray(a, dtype=np.float32) for a in Y], axis=1) for Y in probs])
        p = np.ascontiguousarray(probs, dtype=np.float32)
        if p.ndim != 3 or p.shape[2] != 90:
            raise ValueError("ensemble_average: probs must be [K, n, 90], got %r" % (p.shape,))
        out = np.empty(p.shape[1:], dtype=np.float32)
        self._check(self._lib.clair_ensemble_average(self._h, int(slot), _ptr(p), p.shape[0], p.shape[1], _ptr(out)), "clair_ensemble_average")
        return out

    # -- ensemble across BAMs (include/clair_amd.h: clair_sites_*) --------------------------------------
    def site_table(self):
        """clair_sites_create: a SiteTable of this handle."""
        import weakref
        table = SiteTable(self)
        self._tables.append(weakref.ref(table))
        return table

    def submit_sites(self, slot, table, first, batch, centre, seq, counts=False):
        """clair_submit_sites: every checkpoint of the handle over the batch (as submit_calls takes it), folded into `table` as candidates
        [first, first + n) of its current source; centre uint8 [n,2], seq uint8 [n,33] / [n,34].  wait(slot) returns None."""
        from clair_amd._hostapi import site_seq_bytes
        keep, ptr, is_counts, stride, n = prepare_batch(batch, counts)
        c = np.ascontiguousarray(centre, dtype=np.uint8)
        q = site_seq_bytes(seq)
        if c.shape != (n, 2) or q.shape != (n, 33):
            raise ValueError("centre must be uint8 [%d,2] and seq uint8 [%d,33], got %r and %r" % (n, n, c.shape, q.shape))
        self._check(self._lib.clair_submit_sites(self._h, int(slot), table._h, int(first), ptr, is_counts, stride, n, _ptr(c), _ptr(q)), "clair_submit_sites")
        self._pending[slot] = ((keep, c, q, table), None)

    def submit_site_calls(self, slot, table, first, n, with_calls=True, with_probabilities=False):
        """clair_submit_site_calls: the decode of entries [first, first + n) of the table's output list.  wait(slot) returns what it returns
        after submit_ensemble: the call records, (records, [gt21, genotype, len1, len2]), or the four arrays alone with with_calls=False."""
        from clair_amd._hostapi import CALL_DTYPE
        calls = np.zeros(n, dtype=CALL_DTYPE) if with_calls else None
        outs = self._alloc_out(n) if with_probabilities or calls is None else None
        ptrs = [_ptr(o) for o in outs] if outs else [None] * 4
        self._check(self._lib.clair_submit_site_calls(self._h, int(slot), table._h, int(first), int(n), _ptr(calls) if calls is not None else None, *ptrs),
                    "clair_submit_site_calls")
        self._pending[slot] = ((table,), outs if calls is None else ((calls, outs) if outs else calls))

    def pinned_buffer(self, nbytes):
        """A page-locked uint8 array of nbytes (clair_pinned_alloc): data placed in it -- e.g. read from a file with readinto -- goes to
        the GPU from where it lies when a view INTO it is handed to submit_calls.  It lives as long as the engine."""
        p = ctypes.c_void_p()
        self._check(self._lib.clair_pinned_alloc(self._h, int(nbytes), ctypes.byref(p)), "clair_pinned_alloc")
        return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), shape=(int(nbytes),))

    def decode(self, x, Y, centre, slot=0):
        """clair_decode: the device decode on given probabilities Y = [gt21, genotype, len1, len2] -> call records."""
        from clair_amd._hostapi import CALL_DTYPE
        x = self._prep_x(x)
        n = x.shape[0]
        ys = [np.ascontiguousarray(a, dtype=np.float32) for a in Y]
        c = np.ascontiguousarray(centre, dtype=np.uint8)
        if c.shape != (n, 2) or [a.shape for a in ys] != [(n, 21), (n, 3), (n, 33), (n, 33)]:
            raise ValueError("decode: shapes do not match %d candidates" % n)
        calls = np.zeros(n, dtype=CALL_DTYPE)
        self._check(self._lib.clair_decode(self._h, int(slot), _ptr(x), *[_ptr(a) for a in ys], n, _ptr(c), _ptr(calls)), "clair_decode")
        return calls

    # -- scoring against truth labels (include/clair_amd.h: clair_eval_*) --------------------------
    @staticmethod
    def _prep_labels(labels, n):
        lab = np.ascontiguousarray(labels, dtype=np.uint8)
        if lab.shape != (n, 4):
            raise ValueError("labels must be uint8 [%d,4] (gt21, genotype, len1, len2 true indices), got %r" % (n, lab.shape))
        return lab

    def eval_reset(self):
        """clair_eval_reset: zero the handle's confusion counters."""
        self._check(self._lib.clair_eval_reset(self._h), "clair_eval_reset")

    def submit_eval(self, slot, batch, labels, counts=False, with_probabilities=False):
        """clair_submit_eval: forward pass + scoring against `labels` (uint8 [n,4]) on the device.  batch as submit_calls takes it
        ([n,33,8,4] float32, raw int16 counts with counts=True, or (device address, n) of int16 counts).  wait(slot) returns None, or
        [gt21, genotype, len1, len2] with with_probabilities=True; the counters come from eval_read()."""
        x, ptr, is_counts, stride, n = prepare_batch(batch, counts)
        lab = self._prep_labels(labels, n)
        outs = self._alloc_out(n) if with_probabilities else None
        ptrs = [_ptr(o) for o in outs] if outs else [None] * 4
        self._check(self._lib.clair_submit_eval(self._h, int(slot), ptr, is_counts, stride, n, _ptr(lab), *ptrs), "clair_submit_eval")
        self._pending[slot] = ((x, lab), outs)

    def eval_probabilities(self, Y, labels, slot=0):
        """clair_eval: the device scoring alone on given probabilities Y = [gt21, genotype, len1, len2]."""
        ys = [np.ascontiguousarray(a, dtype=np.float32) for a in Y]
        n = ys[0].shape[0]
        if [a.shape for a in ys] != [(n, 21), (n, 3), (n, 33), (n, 33)]:
            raise ValueError("eval_probabilities: shapes do not match %d candidates" % n)
        lab = self._prep_labels(labels, n)
        self._check(self._lib.clair_eval(self._h, int(slot), *[_ptr(a) for a in ys], _ptr(lab), n), "clair_eval")

    def eval_read(self):
        """clair_eval_read: the counter block, int64 [EVAL_COUNTS] (clair_amd.evaluate.split_counts names its parts)."""
        out = np.zeros(EVAL_COUNTS, dtype=np.int64)
        self._check(self._lib.clair_eval_read(self._h, _ptr(out)), "clair_eval_read")
        return out

    def slot_input(self, slot):
        """The slot's page-locked input buffer as a NumPy array [max_batch,33,8,4] float32: fill rows [0,n) and submit
        `buf[:n]` for a direct DMA transfer instead of the staged copy pageable arrays get."""
        p = ctypes.c_void_p()
        self._check(self._lib.clair_slot_input(self._h, int(slot), ctypes.byref(p)), "clair_slot_input")
        n = self.max_batch * 1056
        return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_float)), shape=(n,)).reshape(self.max_batch, 33, 8, 4)

    def wait(self, slot):
        self._check(self._lib.clair_wait(self._h, slot), "clair_wait")
        _, outs = self._pending.pop(slot)
        return outs

    # -- resident data sets ------------------------------------------------------------------
    def dataset_alloc(self, n):
        xd, od = ctypes.c_void_p(), ctypes.c_void_p()
        self._check(self._lib.clair_dataset_alloc(self._h, int(n), ctypes.byref(xd), ctypes.byref(od)), "clair_dataset_alloc")
        return xd, od

    def dataset_free(self, xd, od):
        self._check(self._lib.clair_dataset_free(self._h, xd, od), "clair_dataset_free")

    def dataset_upload(self, xd, first, x):
        x = self._prep_x(x)
        self._check(self._lib.clair_dataset_upload(self._h, xd, int(first), _ptr(x), x.shape[0]), "clair_dataset_upload")

    def dataset_download(self, od, first, n):
        out = np.empty((n, 90), dtype=np.float32)
        self._check(self._lib.clair_dataset_download(self._h, od, int(first), _ptr(out), int(n)), "clair_dataset_download")
        return out

    def run_resident(self, slot, xd, od, first, n):
        self._check(self._lib.clair_run_resident(self._h, int(slot), xd, od, int(first), int(n)), "clair_run_resident")

    def sync(self):
        self._check(self._lib.clair_sync(self._h), "clair_sync")

    # -- measurement ---------------------------------------------------------------------------
    def timing_enable(self, on=True, only=None):
        """HIP-event timing of every kernel (on=True), of none (False), or of the kernels named in `only` (KERNEL_NAMES)."""
        mask = int(bool(on))
        if only:
            mask = 0
            for k in only:
                mask |= 1 << KERNEL_NAMES.index(k)
        self._check(self._lib.clair_timing_enable(self._h, mask), "clair_timing_enable")

    def timing_reset(self):
        self._check(self._lib.clair_timing_reset(self._h), "clair_timing_reset")

    def kernel_times(self):
        ms = np.zeros(len(KERNEL_NAMES), dtype=np.float64)
        cnt = np.zeros(len(KERNEL_NAMES), dtype=np.int64)
        self._check(self._lib.clair_kernel_times(self._h, _ptr(ms), _ptr(cnt)), "clair_kernel_times")
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(KERNEL_NAMES)}

    def kernel_workgroups(self, n):
        """Workgroups each kernel is launched with for a batch of n candidates (its share of the 256 CUs)."""
        wg = np.zeros(len(KERNEL_NAMES), dtype=np.int32)
        self._check(self._lib.clair_kernel_workgroups(self._h, int(n), _ptr(wg)), "clair_kernel_workgroups")
        return {k: int(wg[i]) for i, k in enumerate(KERNEL_NAMES)}

    def counter(self, name):
        """Event counters of the handle: "fused_launches", "fused_recoveries" (include/clair_amd.h: clair_engine_counter)."""
        v = ctypes.c_int64()
        self._check(self._lib.clair_engine_counter(self._h, ("fused_launches", "fused_recoveries").index(name), ctypes.byref(v)), "clair_engine_counter")
        return int(v.value)

    def debug_read(self, slot, which, shape):
        out = np.empty(shape, dtype=np.float32)
        self._check(self._lib.clair_debug_read(self._h, int(slot), int(which), _ptr(out), out.size), "clair_debug_read")
        return out


class SiteTable(DeviceHandle):
    """clair_sites_*: the site table of ensemble calling across BAMs, in device memory (csrc/sites.hip.h; docs/ensemble.md).  Made by
    Engine.site_table(); its errors are the engine's.  Same methods as clair_amd._hostapi.HostSiteTable, its CPU twin; the batches of a run
    go in through Engine.submit_sites, the decode of the output list comes out of Engine.submit_site_calls."""

    def __init__(self, engine):
        self._lib = engine._lib
        self._engine = engine
        out = self._own(self._lib.clair_sites_destroy, self._lib.clair_last_error)
        engine._check(self._lib.clair_sites_create(engine._h, out), "clair_sites_create")
        self.n_out = 0

    def _check(self, rc, what):
        if rc != 0:
            raise EngineError("%s failed: %s" % (what, self._last_error(self._engine._h).decode()))

    def begin_source(self, positions):
        """-> how many of the positions (int64, strictly ascending) the table did not have"""
        p = np.ascontiguousarray(positions, dtype=np.int64)
        n_new = ctypes.c_int64(0)
        self._check(self._lib.clair_sites_begin_source(self._h, _ptr(p), len(p), ctypes.byref(n_new)), "clair_sites_begin_source")
        return int(n_new.value)

    def add_rows(self, first, probs, x=None, centre=None, seq=None):
        """clair_sites_add_rows: one run's packed rows [n,90] for candidates [first, first + n) of the current source (n <= max_batch)."""
        from clair_amd._hostapi import site_rows_arguments
        n = len(probs)
        p, x, centre, seq = site_rows_arguments(n, probs, x, centre, seq)
        self._check(self._lib.clair_sites_add_rows(self._engine._h, self._h, int(first), _ptr(p), n, *[_ptr(a) if a is not None else None for a in (x, centre, seq)]),
                    "clair_sites_add_rows")

    def finish(self, min_count=0, order="chain"):
        from clair_amd._hostapi import SITE_ORDERS
        n_out = ctypes.c_int64(0)
        self._check(self._lib.clair_sites_finish(self._h, int(min_count), SITE_ORDERS.index(order), ctypes.byref(n_out)), "clair_sites_finish")
        self.n_out = int(n_out.value)
        return self.n_out

    def info(self, first, n):
        """-> (positions int64 [n], counts int32 [n], seq uint8 [n,34] NUL-terminated) of entries [first, first + n) of the output list"""
        positions, counts, seq = np.empty(n, np.int64), np.empty(n, np.int32), np.zeros((n, 33), np.uint8)
        self._check(self._lib.clair_sites_info(self._h, int(first), int(n), _ptr(positions), _ptr(counts), _ptr(seq)), "clair_sites_info")
        return positions, counts, np.concatenate([seq, np.zeros((n, 1), np.uint8)], axis=1)

    def rows(self, first, n):
        out = np.empty((n, 90), dtype=np.float32)
        self._check(self._lib.clair_sites_rows(self._h, int(first), int(n), _ptr(out)), "clair_sites_rows")
        return out

    def windows(self, first, n):
        x = np.empty((n, 33, 8, 4), dtype=np.float32)
        self._check(self._lib.clair_sites_windows(self._h, int(first), int(n), _ptr(x)), "clair_sites_windows")
        return x


def split_outputs(packed):
    """[n,90] packed rows -> [gt21, genotype, len1, len2] (copies, C-contiguous)."""
    return [np.ascontiguousarray(packed[:, a:b]) for a, b in ((0, 21), (21, 24), (24, 57), (57, 90))]


class MalformedText(EngineError):
    pass


class TalliesIncomplete(EngineError):
    """clair_frontend_gvcf_blocks: the front end reported a CLAIR_FE_* bit, so the device does not band its tallies (the host twin runs)."""


class BadArgument(EngineError):
    """A verdict on an argument (return code 2): the handle stays usable; str() is the library's text, the same on both backends."""


class MalformedRecord(EngineError):
    """clair_frontend_add_bam: a BAM record whose sizes do not fit its block_size; .index = its index in the chunk."""

    def __init__(self, msg, index):
        EngineError.__init__(self, msg)
        self.index = index


class DeviceWindows(object):
    """n pileup windows [33][8][4] int16 in device memory (clair_frontend_counts_device): what Engine.submit_calls takes in place of a
    host array.  Keeps its Frontend alive; host() copies the counts back (the decode needs them only when a BAM is consulted)."""

    def __init__(self, frontend, first, n):
        self.frontend, self.first, self.n = frontend, int(first), int(n)
        self.address = frontend.counts_address(first)

    def __len__(self):
        return self.n

    def host(self):
        return self.frontend.window_counts(self.first, self.n)


class Frontend(DeviceHandle):
    """Thin object wrapper over one clair_frontend_t (include/clair_amd.h, "front end on the device")."""

    def __init__(self, device, reference_sequence, reference_start_0_based, span_lo, span_hi, lib_path=None):
        self._lib = load(lib_path)
        ref = reference_sequence.encode("latin-1") if isinstance(reference_sequence, str) else bytes(reference_sequence)
        out = self._own(self._lib.clair_frontend_destroy, self._lib.clair_frontend_last_error)
        self._check(self._lib.clair_frontend_create(int(device), ref, len(ref), int(reference_start_0_based), int(span_lo), int(span_hi), out),
                    "clair_frontend_create")
        self.slab_reads = []                # host copies of each slab's read records: the budget replay walks them

    def add_slab(self, packer):
        """Send the slab a clair_amd._hostapi.SamPacker is holding to the device and start the next one."""
        (r, o, e, q), st = packer.slab_pointers()
        if st["reads"] and st["ops"]:
            from clair_amd._hostapi import READ_DTYPE
            self._check(self._lib.clair_frontend_add_reads(self._h, r, st["reads"], o, st["ops"], e, q, st["seq_bytes"]), "clair_frontend_add_reads")
            buf = (ctypes.c_char * (st["reads"] * READ_DTYPE.itemsize)).from_address(r)
            self.slab_reads.append(np.frombuffer(buf, dtype=READ_DTYPE).copy())
        packer.reset()

    def add_arrays(self, reads, ops, op_elem, seq):
        """The same from NumPy arrays (tests)."""
        from clair_amd._hostapi import OP_DTYPE, READ_DTYPE
        reads = np.ascontiguousarray(reads, dtype=READ_DTYPE)
        ops = np.ascontiguousarray(ops, dtype=OP_DTYPE)
        op_elem = np.ascontiguousarray(op_elem, dtype=np.uint32)
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        if len(reads) and len(ops):
            self._check(self._lib.clair_frontend_add_reads(self._h, _ptr(reads), len(reads), _ptr(ops), len(ops), _ptr(op_elem), _ptr(seq), len(seq)),
                        "clair_frontend_add_reads")
            self.slab_reads.append(reads.copy())

    def text_options(self, ctg_name, dcov=250, evc_min_mq=0, pile_min_mq=0, pile_region=None):
        """What clair_amd._hostapi.SamPacker takes: from here on add_text() does the packing on the device."""
        a, b = (-1, -1) if pile_region is None else (int(pile_region[0]), int(pile_region[1]))
        self._check(self._lib.clair_frontend_text_options(self._h, ctg_name.encode(), int(dcov), int(evc_min_mq), int(pile_min_mq), a, b),
                    "clair_frontend_text_options")

    def add_text(self, sam, length=None):
        """`samtools view` text, whole lines: bytes, or (address, length) of a buffer -- e.g. a page-locked one of the engine the pipe was
        read into.  Raises MalformedText when a line is not an alignment line (the host packer on the same text says which and why)."""
        if length is None:
            address, length = ctypes.cast(ctypes.c_char_p(sam), ctypes.c_void_p).value, len(sam)
        else:
            address = int(sam)
        before = self.stats()["slabs"]
        rc = self._lib.clair_frontend_add_text(self._h, address, int(length))
        if rc == 2:
            raise MalformedText(self._last_error(self._h).decode())
        self._check(rc, "clair_frontend_add_text")
        self._keep_slab_reads(before)

    def _keep_slab_reads(self, before):
        if self.stats()["slabs"] > before:
            from clair_amd._hostapi import READ_DTYPE
            n = ctypes.c_int64(0)
            self._check(self._lib.clair_frontend_slab_reads(self._h, before, None, 0, ctypes.byref(n)), "clair_frontend_slab_reads")
            reads = np.empty(n.value, dtype=READ_DTYPE)
            self._check(self._lib.clair_frontend_slab_reads(self._h, before, _ptr(reads), n.value, ctypes.byref(n)), "clair_frontend_slab_reads")
            self.slab_reads.append(reads)

    def bam_options(self, tid, dcov=250, evc_min_mq=0, pile_min_mq=0, pile_region=None, region=None):
        """The binary twin of text_options: records of reference id `tid`; region = (lo, hi) of `samtools view <bam> ctg:lo-hi` (None: the
        whole contig), pile_region as text_options'.  From here on add_bam() feeds the front end."""
        a, b = (-1, -1) if pile_region is None else (int(pile_region[0]), int(pile_region[1]))
        lo, hi = (-1, -1) if region is None else (int(region[0]), int(region[1]))
        self._check(self._lib.clair_frontend_bam_options(self._h, int(tid), int(dcov), int(evc_min_mq), int(pile_min_mq), a, b, lo, hi),
                    "clair_frontend_bam_options")

    def bam_lookup(self, keep=True):
        """clair_frontend_bam_lookup, after bam_options: keep and mark what the indel look-up counts (indel_table)."""
        self._check(self._lib.clair_frontend_bam_lookup(self._h, 1 if keep else 0), "clair_frontend_bam_lookup")

    def bam_subsample(self, seed, frac):
        """clair_frontend_bam_subsample, after bam_options and before the first record: add_bam also drops what `samtools view -s` would
        (docs/subsample.md); frac <= 0: off."""
        self._check(self._lib.clair_frontend_bam_subsample(self._h, int(seed), float(frac)), "clair_frontend_bam_subsample")

    def indel_table(self, positions, capacity=32):
        """clair_frontend_indel_table: the indel tables of `positions` (1-based, strictly ascending) from the resident slabs, in one device
        call -> entries [n][capacity] (clair_amd._hostapi.ENTRY_DTYPE), n_entries, depth (int32), status (uint32, CLAIR_LOOKUP_*)."""
        from clair_amd._hostapi import ENTRY_DTYPE
        positions = np.ascontiguousarray(positions, dtype=np.int64)
        n = len(positions)
        entries = np.zeros((n, int(capacity)), dtype=ENTRY_DTYPE)
        n_entries, depth, status = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint32)
        self._check(self._lib.clair_frontend_indel_table(self._h, _ptr(positions), n, _ptr(entries), int(capacity), _ptr(n_entries), _ptr(depth), _ptr(status)),
                    "clair_frontend_indel_table")
        return entries, n_entries, depth, status

    def add_bam(self, records, length, offsets, n_records):
        """Whole BAM records (clair_amd._hostapi.BamReader.readinto): records = address (int) or a uint8 array, offsets an int64 array of
        their starts.  Raises MalformedRecord (with .index) when a record's sizes do not fit its block_size."""
        address = int(records) if isinstance(records, int) else records.ctypes.data
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        before = self.stats()["slabs"]
        rc = self._lib.clair_frontend_add_bam(self._h, address, int(length), _ptr(offsets), int(n_records))
        if rc == 2:
            import re
            msg = self._last_error(self._h).decode()
            m = re.search(r"record (\d+)", msg)
            raise MalformedRecord(msg, int(m.group(1)) if m else 0)
        self._check(rc, "clair_frontend_add_bam")
        self._keep_slab_reads(before)

    def text_stats(self):
        v = (ctypes.c_int64 * 4)()
        self._check(self._lib.clair_frontend_text_stats(self._h, v), "clair_frontend_text_stats")
        return dict(zip(("lines", "evc_reads", "pile_reads", "anomalies"), [int(x) for x in v]))

    def find_candidates(self, min_coverage=4, threshold=0.125, ctg_start=None, ctg_end=None, bed=None):
        have_range = ctg_start is not None and ctg_end is not None
        if bed is None:
            bs = be = np.zeros(0, dtype=np.int64)
            n_bed = -1
        else:
            bs = np.ascontiguousarray([b[0] for b in bed], dtype=np.int64)
            be = np.ascontiguousarray([b[1] for b in bed], dtype=np.int64)
            n_bed = len(bs)
        n = ctypes.c_int64(0)
        self._check(self._lib.clair_frontend_find_candidates(self._h, float(min_coverage), float(threshold), int(ctg_start) if have_range else -1,
                                                             int(ctg_end) if have_range else -1, _ptr(bs), _ptr(be), n_bed, ctypes.byref(n)),
                    "clair_frontend_find_candidates")
        return int(n.value)

    def set_candidates(self, positions):
        p = np.ascontiguousarray(positions, dtype=np.int64)
        n = ctypes.c_int64(0)
        self._check(self._lib.clair_frontend_set_candidates(self._h, _ptr(p), len(p), ctypes.byref(n)), "clair_frontend_set_candidates")
        return int(n.value)

    def candidates(self):
        out = np.empty(max(self.stats()["candidates"], 0), dtype=np.int64)
        self._check(self._lib.clair_frontend_get_candidates(self._h, _ptr(out)), "clair_frontend_get_candidates")
        return out

    def build_windows(self, min_coverage=0, drop_non_iupac_centre=True, consider_left_edge=True):
        n = ctypes.c_int64(0)
        self._check(self._lib.clair_frontend_build_windows_ex(self._h, int(min_coverage), int(bool(drop_non_iupac_centre)), int(bool(consider_left_edge)),
                                                              ctypes.byref(n)), "clair_frontend_build_windows")
        return int(n.value)

    def window_info(self, first, n):
        """-> (centres int64 [n], refseq uint8 [n,34] NUL-padded)"""
        centres = np.empty(n, dtype=np.int64)
        seqs = np.zeros((n, 34), dtype=np.uint8)
        self._check(self._lib.clair_frontend_window_info(self._h, int(first), int(n), _ptr(centres), _ptr(seqs)), "clair_frontend_window_info")
        return centres, seqs

    def window_counts(self, first, n):
        counts = np.empty((n, 33, 8, 4), dtype=np.int16)
        self._check(self._lib.clair_frontend_window_counts(self._h, int(first), int(n), _ptr(counts)), "clair_frontend_window_counts")
        return counts

    @staticmethod
    def _bed_arrays(bed):
        if bed is None:
            z = np.zeros(0, dtype=np.int64)
            return z, z, -1
        return (np.ascontiguousarray([b[0] for b in bed], dtype=np.int64), np.ascontiguousarray([b[1] for b in bed], dtype=np.int64), len(bed))

    def sample_candidates(self, truth, p_near, p_outside, key, min_coverage=4, ctg_start=None, ctg_end=None, bed=None, add_truth=True):
        """clair_frontend_sample_candidates in place of find_candidates: the sampled sites (and the truth sites of the range) become the
        candidate list -> (n_candidates, n_near, n_outside).  truth: 1-based, ascending; key: _hostapi.train_set_key(ctg, seed, 1)."""
        have_range = ctg_start is not None and ctg_end is not None
        bs, be, n_bed = self._bed_arrays(bed)
        t = np.ascontiguousarray(truth, dtype=np.int64)
        n, near, outside = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self._lib.clair_frontend_sample_candidates(self._h, float(min_coverage), int(ctg_start) if have_range else -1, int(ctg_end) if have_range else -1,
                                                               _ptr(bs), _ptr(be), n_bed, _ptr(t), len(t), float(p_near), float(p_outside), int(key),
                                                               int(bool(add_truth)), ctypes.byref(n), ctypes.byref(near), ctypes.byref(outside)),
                    "clair_frontend_sample_candidates")
        return int(n.value), int(near.value), int(outside.value)

    def pair(self, truth, truth_labels, amp, key, bed=None):
        """clair_frontend_pair over the windows of build_windows -> dict(v, c, kept_var, kept_non, in_set); key of stage 2."""
        bs, be, n_bed = self._bed_arrays(bed)
        t = np.ascontiguousarray(truth, dtype=np.int64)
        tl = np.ascontiguousarray(truth_labels, dtype=np.uint8).reshape(len(t), 4)
        stats = np.zeros(5, dtype=np.int64)
        self._check(self._lib.clair_frontend_pair(self._h, _ptr(t), _ptr(tl), len(t), _ptr(bs), _ptr(be), n_bed, float(amp), int(key), _ptr(stats)),
                    "clair_frontend_pair")
        return dict(zip(("v", "c", "kept_var", "kept_non", "in_set"), stats.tolist()))

    def train_set_info(self, first, n):
        """-> (centres int64 [n], refseq uint8 [n,34] NUL-padded, labels uint8 [n,4], in_set uint8 [n]) of rows of the kept list"""
        centres, seqs = np.empty(n, dtype=np.int64), np.zeros((n, 34), dtype=np.uint8)
        labels, in_set = np.zeros((n, 4), dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        self._check(self._lib.clair_frontend_train_set_info(self._h, int(first), int(n), _ptr(centres), _ptr(seqs), _ptr(labels), _ptr(in_set)),
                    "clair_frontend_train_set_info")
        return centres, seqs, labels, in_set

    def train_set_counts(self, first, n):
        counts = np.empty((n, 33, 8, 4), dtype=np.int16)
        self._check(self._lib.clair_frontend_train_set_counts(self._h, int(first), int(n), _ptr(counts)), "clair_frontend_train_set_counts")
        return counts

    def counts_address(self, first):
        a = self._lib.clair_frontend_counts_device(self._h, int(first))
        if not a:
            raise EngineError("clair_frontend_counts_device: no windows yet")
        return int(a)

    def stats(self):
        v = (ctypes.c_int64 * 6)()
        self._check(self._lib.clair_frontend_stats(self._h, v), "clair_frontend_stats")
        return dict(zip(("anomalies", "slabs", "reads", "elements", "candidates", "windows"), [int(x) for x in v]))

    def position_tallies(self, first, n):
        """clair_frontend_position_tallies -> uint32 [n, 7]: A C G T I D N of the 0-based positions [first, first + n)"""
        out = np.zeros((max(int(n), 0), 7), dtype=np.uint32)
        rc = self._lib.clair_frontend_position_tallies(self._h, int(first), int(n), _ptr(out))
        if rc == 2:
            raise BadArgument(self._last_error(self._h).decode())
        self._check(rc, "clair_frontend_position_tallies")
        return out

    def gvcf_blocks(self, costs, band_of_gq, iv_start, iv_end, guard=0):
        """clair_frontend_gvcf_blocks -> records (clair_amd.gvcf.BLOCK_DTYPE).  costs = (c_match, c_err, c_half), band_of_gq uint8 [100], the
        allowed intervals as two int64 arrays.  guard: that many further records behind the result, filled with 0xA5 bytes before the call
        (tests look at them afterwards).  Raises BadArgument / TalliesIncomplete for the return codes 2 / 3."""
        from clair_amd.gvcf import BLOCK_DTYPE
        bands = np.ascontiguousarray(band_of_gq, dtype=np.uint8)
        st, en = np.ascontiguousarray(iv_start, dtype=np.int64), np.ascontiguousarray(iv_end, dtype=np.int64)
        if bands.shape != (100,) or st.shape != en.shape or st.ndim != 1:
            raise ValueError("gvcf_blocks: a band table of 100 entries and two interval arrays of one length")
        n = ctypes.c_int64(0)

        def call(out, capacity):
            rc = self._lib.clair_frontend_gvcf_blocks(self._h, int(costs[0]), int(costs[1]), int(costs[2]), _ptr(bands), _ptr(st), _ptr(en), len(st),
                                                      None if out is None else _ptr(out), capacity, ctypes.byref(n))
            if rc in (2, 3):
                raise (BadArgument if rc == 2 else TalliesIncomplete)(self._last_error(self._h).decode())
            self._check(rc, "clair_frontend_gvcf_blocks")
        call(None, 0)
        out = np.empty(n.value + int(guard), dtype=BLOCK_DTYPE)
        out.view(np.uint8)[:] = 0xA5
        if n.value:
            call(out, n.value)
        return out if guard else out[:n.value]

    def gvcf_device_ms(self):
        """clair_frontend_gvcf_device_ms: event time of the launches of the last gvcf_blocks computation"""
        ms = ctypes.c_double(0.0)
        self._check(self._lib.clair_frontend_gvcf_device_ms(self._h, ctypes.byref(ms)), "clair_frontend_gvcf_device_ms")
        return ms.value

    def budget_binds(self, available_slots=5000000):
        """Replay CreateTensor's count of free tuple slots over everything added (clair_host_tuple_budget_binds)."""
        from clair_amd import _hostapi
        n_cand = self.stats()["candidates"]
        centres = np.empty(max(n_cand, 0), dtype=np.int64)
        window_tuples = np.empty(max(n_cand, 0), dtype=np.uint64)
        self._check(self._lib.clair_frontend_budget_inputs(self._h, 0, None, _ptr(centres), _ptr(window_tuples)), "clair_frontend_budget_inputs")
        state = np.array([available_slots, 0], dtype=np.int64)
        for k, reads in enumerate(self.slab_reads):
            tuples = np.empty(len(reads), dtype=np.uint64)
            self._check(self._lib.clair_frontend_budget_inputs(self._h, k, _ptr(tuples), None, None), "clair_frontend_budget_inputs")
            if _hostapi.tuple_budget_binds(reads, tuples, centres, window_tuples, state):
                return True
        return False

    def read_tuples(self, slab):
        tuples = np.empty(len(self.slab_reads[slab]), dtype=np.uint64)
        self._check(self._lib.clair_frontend_budget_inputs(self._h, int(slab), _ptr(tuples), None, None), "clair_frontend_budget_inputs")
        return tuples

    def window_tuples(self):
        n_cand = max(self.stats()["candidates"], 0)
        centres = np.empty(n_cand, dtype=np.int64)
        window_tuples = np.empty(n_cand, dtype=np.uint64)
        self._check(self._lib.clair_frontend_budget_inputs(self._h, 0, None, _ptr(centres), _ptr(window_tuples)), "clair_frontend_budget_inputs")
        return centres, window_tuples


class Inflater(DeviceHandle):
    """clair_inflate_*: BGZF blocks inflated on the device, a wave per block (csrc/inflate.hip).

        inf = Inflater(device=0, max_blocks=2048)
        out, status = inf.blocks(cdata, in_at, csize, out_at, out_len)       # whole BGZF blocks inside cdata -> bytes, status per block

    status: an index into STATUS (_hostapi.INFLATE_STATUS), 0 ok.  `handle` and `callback` are what
    clair_host_bam_set_inflater takes (_hostapi.BamReader(inflate="device"))."""
    STATUS = INFLATE_STATUS

    def __init__(self, device=0, max_blocks=2048):
        self._lib = load()
        out = self._own(self._lib.clair_inflate_destroy, self._lib.clair_inflate_last_error)
        self._check(self._lib.clair_inflate_create(int(device), int(max_blocks), out), "clair_inflate_create")
        self.max_blocks = int(max_blocks)

    @property
    def handle(self):
        return self._h

    @property
    def callback(self):
        return ctypes.cast(self._lib.clair_inflate_blocks_cb, ctypes.c_void_p)

    def blocks(self, cdata, in_at, csize, out_at, out_len, out=None, cbytes=None):
        """-> (out, status): out is a uint8 array (given, or zeros up to the last output range)."""
        cdata = np.frombuffer(cdata, dtype=np.uint8) if not isinstance(cdata, np.ndarray) else cdata
        in_at, out_at = np.ascontiguousarray(in_at, dtype=np.int64), np.ascontiguousarray(out_at, dtype=np.int64)
        csize, out_len = np.ascontiguousarray(csize, dtype=np.int32), np.ascontiguousarray(out_len, dtype=np.int32)
        n = len(in_at)
        if out is None:
            out = np.zeros(int((out_at + out_len).max()) if n else 0, dtype=np.uint8)
        status = np.full(n, -1, dtype=np.int32)
        self._check(self._lib.clair_inflate_blocks(self._h, _ptr(cdata), len(cdata) if cbytes is None else int(cbytes), n, _ptr(in_at), _ptr(csize),
                                                   _ptr(out_at), _ptr(out_len), _ptr(out), _ptr(status)), "clair_inflate_blocks")
        return out, status


class Deflater(DeviceHandle):
    """clair_deflate_*: BGZF blocks compressed on the device, a wave per block (csrc/deflate.hip).

        d = Deflater(device=0, max_blocks=256)
        out, csize = d.blocks(data, in_at, in_len)       # out uint8 [n, 65536]: block i is out[i, :csize[i]]

    The bytes are those of clair_amd._hostapi.deflate_bgzf for the same payload."""

    def __init__(self, device=0, max_blocks=256):
        self._lib = load()
        out = self._own(self._lib.clair_deflate_destroy, self._lib.clair_deflate_last_error)
        self._check(self._lib.clair_deflate_create(int(device), int(max_blocks), out), "clair_deflate_create")
        self.max_blocks = int(max_blocks)

    def blocks(self, data, in_at, in_len):
        data = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
        in_at, in_len = np.ascontiguousarray(in_at, dtype=np.int64), np.ascontiguousarray(in_len, dtype=np.int32)
        n = len(in_at)
        if len(in_len) != n:
            raise ValueError("%d offsets for %d lengths" % (n, len(in_len)))
        out = np.zeros((n, 65536), dtype=np.uint8)
        csize = np.zeros(n, dtype=np.int32)
        self._check(self._lib.clair_deflate_blocks(self._h, _ptr(data) if len(data) else None, len(data), n, _ptr(in_at), _ptr(in_len), _ptr(out), _ptr(csize)),
                    "clair_deflate_blocks")
        return out, csize


class Trainer(DeviceHandle):
    """clair_train_*: the training handle (csrc/train.hip; docs/train.md) -- float32 weights, gradients and optimizer state of the 22 tensors on
    the device, forward + loss + backward over one micro-batch at a time, Adam / momentum steps.  Needs no Engine."""
    OPTIMIZERS = ("Adam", "SGDM")
    LOSSES = ("FocalLoss", "CrossEntropy")
    SETS = ("weights", "gradients", "m", "v")
    MASK_SHAPES = ((33, 256), (192,), (96,), (96,), (96,), (96,))        # per row: LSTM2 (stored [33][n][256]), L4, L5_1..4

    def __init__(self, device=0, micro_batch=1024, optimizer="Adam", loss="FocalLoss", lib_path=None):
        self._lib = load(lib_path)
        self.micro_batch = int(micro_batch)
        self.last_n = 0
        out = self._own(self._lib.clair_train_destroy, self._lib.clair_train_last_error)
        self._check(self._lib.clair_train_create(int(device), int(micro_batch), self.OPTIMIZERS.index(optimizer), self.LOSSES.index(loss), out),
                    "clair_train_create")

    def set_tensors(self, w, which="weights"):
        from clair_amd.weights import TENSOR_IDS, check_weights
        check_weights(w)
        for key, tid in TENSOR_IDS.items():
            a = np.ascontiguousarray(w[key], dtype=np.float32)
            self._check(self._lib.clair_train_set_tensor(self._h, self.SETS.index(which), tid, _ptr(a), a.size), "clair_train_set_tensor(%s)" % key)

    def get_tensors(self, which="weights"):
        from collections import OrderedDict
        from clair_amd.weights import TENSOR_IDS, TENSOR_TABLE
        out = OrderedDict()
        for key, tid in TENSOR_IDS.items():
            a = np.empty(TENSOR_TABLE[key], dtype=np.float32)
            self._check(self._lib.clair_train_get_tensor(self._h, self.SETS.index(which), tid, _ptr(a), a.size), "clair_train_get_tensor(%s)" % key)
            out[key] = a
        return out

    def config(self, task_loss_weights=None, class_weights=None, dropout_rates=None, seed=0):
        """task_loss_weights [5], class_weights [90], dropout_rates [6] (LSTM2, L4, L5_1..4); None keeps what the handle has."""
        arrays = []
        for a, size in ((task_loss_weights, 5), (class_weights, 90), (dropout_rates, 6)):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.float64)
                if a.shape != (size,):
                    raise ValueError("config: an array of %d values expected, got shape %r" % (size, a.shape))
            arrays.append(a)
        self._check(self._lib.clair_train_config(self._h, *([_ptr(a) if a is not None else None for a in arrays] + [int(seed)])), "clair_train_config")

    def zero_grad(self):
        self._check(self._lib.clair_train_zero_grad(self._h), "clair_train_zero_grad")

    def accumulate(self, x, labels, first_row=0, training=True):
        """One micro-batch (n <= micro_batch): x [n,33,8,4], labels uint8 [n,4] -> float64 [4], the heads' losses summed over the rows."""
        x = Engine._prep_x(x)
        lab = Engine._prep_labels(labels, x.shape[0])
        losses = np.zeros(4, dtype=np.float64)
        self._check(self._lib.clair_train_accumulate(self._h, _ptr(x), _ptr(lab), x.shape[0], int(first_row), int(bool(training)), _ptr(losses)),
                    "clair_train_accumulate")
        self.last_n = x.shape[0]
        return losses

    def step(self, learning_rate, l2_lambda):
        """-> (l2 loss without lambda of the weights before the update, global gradient norm before clipping)"""
        stats = np.zeros(2, dtype=np.float64)
        self._check(self._lib.clair_train_step(self._h, float(learning_rate), float(l2_lambda), _ptr(stats)), "clair_train_step")
        return float(stats[0]), float(stats[1])

    def read_mask(self, layer):
        """The mask of the last training accumulate: layer 0 -> uint8 [33,n,256], 1 -> [n,192], 2..5 -> [n,96]."""
        n = self.last_n
        shape = (33, n, 256) if layer == 0 else (n,) + self.MASK_SHAPES[layer]
        out = np.zeros(shape, dtype=np.uint8)
        self._check(self._lib.clair_train_read_mask(self._h, int(layer), _ptr(out), out.size), "clair_train_read_mask")
        return out

    def probabilities(self):
        out = np.empty((self.last_n, 90), dtype=np.float32)
        self._check(self._lib.clair_train_probabilities(self._h, _ptr(out)), "clair_train_probabilities")
        return out

    def accuracy(self):
        """-> int64 [4]: rows of the last accumulate each head gets right (gt21, genotype, smaller and larger of the sorted indel-length pair),
        counted on the device; clair_amd.model.accuracy_counts is the NumPy twin."""
        tp = np.zeros(4, dtype=np.int64)
        self._check(self._lib.clair_train_accuracy(self._h, _ptr(tp)), "clair_train_accuracy")
        return tp

    # -- kernel taps for tests (tests/test_train_kernels_gpu.py): the library checks every address before it launches anything ------------
    def debug_gemm(self, a, b, c, dims, strides, bias=None):
        """One tgemm launch: a, b, c (and bias) flat float32 arrays, dims (M, N, K, batch, accumulate), strides (sam, sak, sbk, sbn, scm, scn,
        ba, bb, bc, bbias) in elements -> the whole of c after the launch, a new array (c itself is left as it is)."""
        a, b = (np.ascontiguousarray(v, dtype=np.float32).ravel() for v in (a, b))
        out = np.array(c, dtype=np.float32, order="C").ravel()
        bias = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32).ravel()
        dims, strides = np.ascontiguousarray(dims, dtype=np.int64), np.ascontiguousarray(strides, dtype=np.int64)
        if dims.shape != (5,) or strides.shape != (10,):
            raise ValueError("debug_gemm: 5 dims and 10 strides expected, got %r and %r" % (dims.shape, strides.shape))
        self._check(self._lib.clair_train_debug_gemm(self._h, _ptr(a), a.size, _ptr(b), b.size, None if bias is None else _ptr(bias), 0 if bias is None else bias.size,
                                                     _ptr(out), out.size, _ptr(dims), _ptr(strides)), "clair_train_debug_gemm")
        return out

    def debug_column_sum(self, x, rows, cols, ld, out, d=1, s1=1, s2=0):
        """One column_sum_kernel launch: out[(j // d) * s1 + (j % d) * s2] += sum over r < rows of x[r * ld + j], j < cols; x and out flat
        float32 arrays -> the whole of out after the launch, a new array."""
        x = np.ascontiguousarray(x, dtype=np.float32).ravel()
        got = np.array(out, dtype=np.float32, order="C").ravel()
        self._check(self._lib.clair_train_debug_column_sum(self._h, _ptr(x), x.size, int(rows), int(cols), int(ld), _ptr(got), got.size, int(d), int(s1), int(s2)),
                    "clair_train_debug_column_sum")
        return got


def overlap_keep(spans, device=0):
    """clair_overlap_keep: spans (clair_amd._hostapi.SPAN_DTYPE [n], input order) -> uint8 [n], 1 for the rows the overlap filter prints, worked
    out on the device (csrc/overlap.hip).  clair_amd._hostapi.overlap_keep gives the same bytes on the CPU."""
    from clair_amd._hostapi import SPAN_DTYPE
    lib = load()
    s = np.ascontiguousarray(spans, dtype=SPAN_DTYPE)
    keep = np.zeros(len(s), dtype=np.uint8)
    if lib.clair_overlap_keep(int(device), _ptr(s), len(s), _ptr(keep)) != 0:
        raise EngineError("clair_overlap_keep failed: %s" % lib.clair_overlap_last_error().decode())
    return keep
