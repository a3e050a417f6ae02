"""Every header of the C ABI against its row of _lib.HEADERS and against the built library, without a GPU: the names, the
signatures argument by argument, the struct mirrors field by field and what lib() bound -- one test id per header.  What
is specific to one header (its C host program, refusals, constants) lives in that header's tests/test_*_abi.py."""
import ctypes
import glob
import os
import re

import pytest
from plnerf_amd import _lib

import abi_support as abi

per_header = pytest.mark.parametrize("header,signatures,mirrors", _lib.HEADERS, ids=[row[0] for row in _lib.HEADERS])


@pytest.fixture(scope="module")
def L():
    return abi.built_lib()


def _path(header):
    return os.path.join(abi.INCLUDE, header)


@per_header
def test_names_agree(L, header, signatures, mirrors):
    """The header declares exactly the entries of its table, and the library exports every one of them."""
    declared = set(abi.prototypes(_path(header)))
    assert declared, "no declarations parsed"
    assert declared == set(signatures), declared ^ set(signatures)
    assert declared <= abi.exported_symbols(L.LIB_PATH), declared - abi.exported_symbols(L.LIB_PATH)


def _check_type(where, c_type, ct):
    """One return or argument type.  A scalar is that ctypes type; a pointer to one of the ABI's structs is POINTER(its
    mirror); `const char*` is c_char_p; any other pointer, or the stream, is c_void_p -- or, where the table declares a host
    array as a typed pointer, a POINTER to the element type the header names."""
    assert abi.ct_class(ct) == abi.c_class(c_type), (where, c_type, ct)
    t = abi.bare(c_type)
    if abi.c_class(c_type) != "ptr":
        assert ct is abi.SCALARS[t], (where, c_type, ct)
        return
    pointee = t[:-1].strip() if t.endswith("*") else None
    if pointee in abi.abi_structs():
        assert ct is ctypes.POINTER(abi.abi_structs()[pointee]), (where, c_type, ct)
    elif c_type == "const char*":
        assert ct is ctypes.c_char_p, (where, c_type, ct)
    elif ct is not ctypes.c_void_p:
        assert pointee, (where, c_type, ct, "the stream is c_void_p")
        element = ctypes.c_void_p if pointee.endswith("*") else abi.SCALARS[pointee]
        assert ct is ctypes.POINTER(element), (where, c_type, ct)


@per_header
def test_signatures_agree(header, signatures, mirrors):
    """The hand-written argument lists restate the header: a swapped c_int / c_float in a 30-argument call would be silent
    undefined behaviour."""
    protos = abi.prototypes(_path(header))
    assert set(protos) == set(signatures)
    for name, (ret, params) in protos.items():
        res, args = signatures[name]
        _check_type((name, "return"), ret, res)
        assert len(args) == len(params), (name, len(args), len(params))
        for k, (c_type, ct) in enumerate(zip(params, args)):
            _check_type((name, k), c_type, ct)


@per_header
def test_struct_mirrors_agree(header, signatures, mirrors):
    """Field names, order, ctypes types and array lengths of every struct the header defines."""
    declared = abi.structs(_path(header))
    assert set(declared) == set(mirrors), set(declared) ^ set(mirrors)
    for name, fields in declared.items():
        mirror = mirrors[name]._fields_
        assert [f[0] for f in mirror] == [f[1] for f in fields], name
        for (fname, ftype), (c_type, _, length) in zip(mirror, fields):
            want = abi.expected_ctype(c_type, length)
            if length is None:
                assert ftype is want, (name, fname, ftype, want)
            else:      # (ctypes array types are cached per (element, length))
                assert ftype._type_ is want._type_ and ftype._length_ == want._length_, (name, fname)


@per_header
def test_binding_agrees(L, header, signatures, mirrors):
    """lib() bound every entry of the table with the table's types."""
    for name, (res, args) in signatures.items():
        fn = getattr(L.lib(), name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_the_registry_is_the_whole_abi(L):
    """Every header under include/ has a row and every row a header; no entry point is declared twice; one ABI version."""
    tables = [signatures for _, signatures, _ in L.HEADERS]
    assert set().union(*tables) == set(L.ALL_SIGNATURES)
    assert sum(len(t) for t in tables) == len(L.ALL_SIGNATURES)      # disjoint over all headers
    for _, signatures, _ in L.HEADERS:
        assert all(L.ALL_SIGNATURES[name] is signature for name, signature in signatures.items())
    on_disk = sorted(os.path.basename(p) for p in glob.glob(os.path.join(abi.INCLUDE, "plnerf_hip*.h")))
    assert on_disk == sorted(header for header, _, _ in L.HEADERS)
    declared = int(re.search(r"#define\s+PLNERF_VERSION\s+(\d+)", open(_path("plnerf_hip.h")).read()).group(1))
    assert declared == L.ABI_VERSION == L.lib().plnerf_version() == 601
