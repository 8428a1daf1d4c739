"""The C-ABI library loads on a GPU-less host and exports every symbol include/clair_amd.h declares."""
import ctypes
import os
import re

import numpy as np
import pytest

from clair_amd import _capi, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "clair_amd.h")


def _declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(clair_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported():
    lib = _capi.load()
    declared = _declared_functions()
    assert declared, "no declarations parsed from the header"
    for name in declared:
        assert hasattr(lib, name), "%s declared in clair_amd.h but not exported" % name
    assert sorted(_capi.SYMBOLS) == declared


RESTYPES = {"void": None, "const char *": ctypes.c_char_p, "void *": ctypes.c_void_p, "int": ctypes.c_int, "int64_t": ctypes.c_int64,
            "uint32_t": ctypes.c_uint32}
SCALARS = {"double": ctypes.c_double, "int64_t": ctypes.c_int64, "int": ctypes.c_int}


def header_prototypes(path, pointer_typedefs=()):
    """{name: (return type, [parameter, ...])} of every prototype of a plain-C header, comments stripped, blanks normalised ("const char *")."""
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    tidy = lambda t: " ".join(t.replace("*", " * ").split())     # noqa: E731
    protos = {}
    for ret, name, params in re.findall(r"^([a-z_0-9 ]+?[ *]+)(clair_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text, flags=re.M):
        params = [tidy(p) for p in params.split(",")]
        protos[name] = (tidy(ret), [] if params == ["void"] else ["* " + p if p.split()[0] in pointer_typedefs else p for p in params])
    return protos


def check_table_against_header(signatures, protos):
    """The rules of a signature table: as many argtypes as parameters, the declared return type, and per parameter a pointer type for a
    pointer, the scalar's own ctypes type otherwise."""
    assert sorted(signatures) == sorted(protos)
    for name, (ret, params) in protos.items():
        restype, argtypes = signatures[name]
        assert len(argtypes) == len(params), "%s: %d argtypes for %r" % (name, len(argtypes), params)
        want = RESTYPES[ret] if ret in RESTYPES else RESTYPES["void *"] if ret.endswith("*") else ret     # any other pointer is an address
        assert restype is want, "%s returns %s, table says %r" % (name, ret, restype)
        for k, (param, argtype) in enumerate(zip(params, argtypes)):
            if "*" in param:
                ok = argtype in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(argtype, ctypes._Pointer)
            else:
                ok = argtype is SCALARS[" ".join(param.split()[:-1])]
            assert ok, "%s: parameter %d is `%s`, table says %r" % (name, k, param, argtype)


def test_signature_table_matches_header():
    protos = header_prototypes(HEADER)
    assert sorted(protos) == _declared_functions()
    check_table_against_header(_capi.SIGNATURES, protos)
    assert _capi.SYMBOLS == tuple(_capi.SIGNATURES)


def test_abi_version_and_tensor_table():
    lib = _capi.load()
    assert lib.clair_abi_version() == 6
    text = open(HEADER).read()
    ids = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"CLAIR_T_([A-Z0-9_]+)\s*=\s*(\d+)", text))
    assert ids.pop("COUNT") == len(weights.TENSOR_TABLE) == 22
    for key, tid in weights.TENSOR_IDS.items():
        assert ids[key.upper()] == tid
    assert weights.N_PARAMS == 2377818


def test_create_fails_loudly_without_device():
    lib = _capi.load()
    if lib.clair_device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(_capi.EngineError) as ei:
        _capi.Engine(device=0, max_batch=16, n_slots=1)
    assert "no HIP device" in str(ei.value)


def test_create_argument_validation():
    lib = _capi.load()
    h = ctypes.c_void_p()
    assert lib.clair_engine_create(0, 0, 1, ctypes.byref(h)) != 0
    assert b"max_batch" in lib.clair_last_error(None)
    assert lib.clair_engine_create(0, 16, 0, ctypes.byref(h)) != 0
    assert b"n_slots" in lib.clair_last_error(None)
    assert not h.value


# -- prepare_batch: what the submit wrappers hand to the library, worked out without loading it ---------------------------------------------
def _address(a):
    return a.ctypes.data


@pytest.mark.parametrize("n", [1, 3])
def test_prepare_batch_dense_float32_goes_as_it_is(n):
    x = np.zeros((n, 33, 8, 4), dtype=np.float32)
    keep, ptr, is_counts, stride, got_n = _capi.prepare_batch(x, False)
    assert keep is x and ptr.value == _address(x) and (is_counts, stride, got_n) == (0, 0, n)


def test_prepare_batch_counts_column_of_records_is_not_copied():
    from clair_amd.tensor_binary import RECORD
    rec = np.zeros(3, dtype=RECORD)
    col = rec["counts"]
    keep, ptr, is_counts, stride, n = _capi.prepare_batch(col, True)
    assert keep is col and ptr.value == _address(col) and (is_counts, stride, n) == (1, RECORD.itemsize, 3)
    one = rec[:1]["counts"]                      # a one-row view is C-contiguous: dense
    keep, ptr, is_counts, stride, n = _capi.prepare_batch(one, True)
    assert keep is one and ptr.value == _address(one) and (is_counts, stride, n) == (1, 0, 1)


@pytest.mark.parametrize("given,counts,dtype", [(np.float64, False, np.float32), (np.float32, True, np.int16)])
def test_prepare_batch_converts_another_dtype(given, counts, dtype):
    x = np.arange(2 * 1056, dtype=given).reshape(2, 33, 8, 4)
    keep, ptr, is_counts, stride, n = _capi.prepare_batch(x, counts)
    assert keep is not x and keep.dtype == dtype and keep.flags.c_contiguous and np.array_equal(keep, x)
    assert ptr.value == _address(keep) and (is_counts, stride, n) == (int(counts), 0, 2)


def test_prepare_batch_rejects_another_shape():
    with pytest.raises(ValueError) as ei:
        _capi.prepare_batch(np.zeros((2, 33, 8, 3), dtype=np.float32), False)
    assert str(ei.value) == "batch must have shape [n,33,8,4], got (2, 33, 8, 3)"


def test_prepare_batch_device_forms():
    class FakeFrontend(object):
        def counts_address(self, first):
            return 0x7000 + first * 2112

    w = _capi.DeviceWindows(FakeFrontend(), 2, 5)
    keep, ptr, is_counts, stride, n = _capi.prepare_batch(w, False)
    assert keep is w and (ptr.value, is_counts, stride, n) == (0x7000 + 2 * 2112, 1, 0, 5)
    keep, ptr, is_counts, stride, n = _capi.prepare_batch((0x9000, 7), True)
    assert keep is None and (ptr.value, is_counts, stride, n) == (0x9000, 1, 0, 7)
