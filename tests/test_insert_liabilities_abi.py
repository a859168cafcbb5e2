"""dapol_tree_derive_leaves / dapol_tree_insert_liabilities at the ABI: both are declared, exported and bound by capi.py, and their
null-argument refusals need no device.  (What they compute: tests/test_gpu_insert_liabilities.py.)"""
import ctypes
import inspect
import os
import re

from conftest import ROOT

NEW = ("dapol_tree_derive_leaves", "dapol_tree_insert_liabilities")
INVALID_ARGUMENT = 8


def test_both_calls_are_declared_exported_and_bound(hip_lib):
    hdr = open(os.path.join(ROOT, "include", "dapol_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = hip_lib.lib()
    for name in NEW:
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, code), name + " is not declared in dapol_hip.h"
        assert hasattr(lib, name), "missing export " + name
        assert name in hip_lib.EXPORTED_SYMBOLS
        assert getattr(lib, name).restype is ctypes.c_int32
    # the header says what the library cannot see: ids the tree already carries
    doc = hdr[hdr.index("build_leaf_nodes for k liabilities that JOIN"):hdr.index("int32_t dapol_tree_derive_leaves")]
    assert "holds no ids" in doc and "insert_liabilities" in doc
    assert len(lib.dapol_tree_derive_leaves.argtypes) == 15 and len(lib.dapol_tree_insert_liabilities.argtypes) == 11


def test_null_arguments_are_refused_without_a_device(hip_lib):
    lib = hip_lib.lib()
    seed = ctypes.create_string_buffer(b"audit")
    off = (ctypes.c_uint32 * 2)(0, 1)
    ids = ctypes.create_string_buffer(b"a")
    val = (ctypes.c_uint64 * 1)(5)
    out8 = (ctypes.c_uint64 * 1)()
    out32 = ctypes.create_string_buffer(32)
    ord4 = (ctypes.c_uint32 * 1)()
    # no tree
    assert lib.dapol_tree_derive_leaves(None, 0, seed, 5, 1, ids, off, ids, off, val, out8, out8, out32, ord4, out8) == INVALID_ARGUMENT
    assert b"null argument" in lib.dapol_last_error()
    assert lib.dapol_tree_insert_liabilities(None, 0, seed, 5, 1, ids, off, ids, off, val, out8) == INVALID_ARGUMENT
    assert b"null argument" in lib.dapol_last_error()
    # ... also for an empty batch, and whatever the digest
    assert lib.dapol_tree_derive_leaves(None, 0, seed, 5, 0, None, None, None, None, None, None, None, None, None, None) == INVALID_ARGUMENT
    assert lib.dapol_tree_insert_liabilities(None, 2, seed, 5, 0, None, None, None, None, None, None) == INVALID_ARGUMENT


def test_capi_wrappers_take_the_list_of_tuples_form(hip_lib):
    for name in ("derive_leaves", "insert_liabilities"):
        sig = inspect.signature(getattr(hip_lib.Tree, name))
        assert list(sig.parameters) == ["self", "liabilities", "audit_seed", "digest"]
        assert sig.parameters["digest"].default == hip_lib.DIGEST_BLAKE3
    n, ib, ioff, eb, eoff, vals, sd = hip_lib._pack_liabilities([(b"ab", b"x", 3), (b"", b"yz", 4)], b"s")
    assert (n, bytes(ib), list(ioff), bytes(eb), list(eoff), list(vals), bytes(sd)) == (2, b"ab", [0, 2, 2], b"xyz", [0, 1, 3], [3, 4], b"s")
