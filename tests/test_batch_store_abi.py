"""dapol_batch_store_* in the C ABI, without a device: declared, exported and bound in every layer; a NULL store, or a creation without a
context, is an invalid argument that writes nothing and does not crash."""
import ctypes
import os

import numpy as np

from conftest import ROOT
from test_abi import declared_symbols

SYMBOLS = ["dapol_batch_store_create", "dapol_batch_store_destroy", "dapol_batch_store_refresh", "dapol_batch_store_rows", "dapol_batch_store_layout",
           "dapol_batch_store_fetch", "dapol_batch_store_read", "dapol_batch_store_verify"]


def test_the_store_is_declared_exported_and_bound(hip_lib):
    for s in SYMBOLS:
        assert s in declared_symbols(), s
        assert hasattr(hip_lib.lib(), s), s
        assert s in hip_lib.EXPORTED_SYMBOLS, s
    for m in ("refresh", "layout", "fetch", "read", "verify", "close"):
        assert callable(getattr(hip_lib.BatchStore, m, None)), m
    assert isinstance(hip_lib.BatchStore.rows, property)


def test_the_cpp_wrapper_the_kernels_and_the_plan_exist():
    hpp = open(os.path.join(ROOT, "include", "dapol.hpp")).read()
    assert "class BatchProofStore" in hpp and "BatchProofStore batch_store(const Bytes32& nonce_seed" in hpp and "dapol_batch_store_create(" in hpp
    assert "BatchProofStore(const BatchProofStore&) = delete;" in hpp
    csrc = os.path.join(ROOT, "dapol_amd", "csrc")
    kernels = open(os.path.join(csrc, "kernels_batch_store.h")).read()
    for k in ("k_batch_store_move", "k_batch_store_fetch"):
        assert "void " + k + "(" in kernels, k
    assert "__shared__" not in kernels and "atomic" not in kernels.lower().replace("no atomics", "")
    plan = open(os.path.join(csrc, "batch_store_plan.inc")).read()
    for f in ("batch_store_match(", "batch_store_same_list(", "batch_store_fetch_offsets(", "batch_store_row(", "batch_store_piece_src("):
        assert f in plan, f
    assert "hip" not in plan.replace("__HIPCC__", "").lower().replace("no hip call", "")
    main = open(os.path.join(csrc, "dapol_hip.hip")).read()
    assert '#include "host_batch_store.inc"' in main and '#include "kernels_batch_store.h"' in main
    assert "#include" not in open(os.path.join(csrc, "host_batch_store.inc")).read()


def test_a_null_store_is_an_invalid_argument_and_writes_nothing(hip_lib):
    lib = hip_lib.lib()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    off, idx, rows = np.array([0, 1], np.uint64), np.array([5], np.uint64), np.array([0], np.uint64)
    out, seed = np.full(4096, 0xAB, np.uint8), np.zeros(32, np.uint8)
    counters = [ctypes.c_uint64(11 * (i + 1)) for i in range(4)]
    assert lib.dapol_batch_store_refresh(None, 1, p(off), p(idx), *[ctypes.byref(c) for c in counters]) == 8
    assert b"null" in lib.dapol_last_error()
    assert lib.dapol_batch_store_refresh(None, 0, None, None, *[ctypes.byref(c) for c in counters]) == 8
    assert [c.value for c in counters] == [11, 22, 33, 44]
    assert lib.dapol_batch_store_layout(None, p(out), p(out), p(out), p(out)) == 8
    assert lib.dapol_batch_store_layout(None, None, None, None, None) == 8
    assert lib.dapol_batch_store_fetch(None, 1, p(rows), p(out), p(out), p(out)) == 8
    assert lib.dapol_batch_store_fetch(None, 0, None, None, None, None) == 8
    assert lib.dapol_batch_store_read(None, 0, 1, p(out), p(out), p(out)) == 8
    assert lib.dapol_batch_store_read(None, 0, 0, None, None, None) == 8
    assert lib.dapol_batch_store_verify(None, p(seed), p(out)) == 8
    assert lib.dapol_batch_store_verify(None, None, p(out)) == 8
    assert (out == 0xAB).all() and idx[0] == 5 and off.tolist() == [0, 1]
    assert lib.dapol_batch_store_rows(None) == 0
    assert lib.dapol_batch_store_destroy(None) == 0                       # as every destroy of the ABI


def test_creation_without_a_context_is_an_error_code_and_no_crash(hip_lib):
    lib = hip_lib.lib()
    seed = np.zeros(32, np.uint8)
    h = ctypes.c_void_p(0x1234)
    assert lib.dapol_batch_store_create(None, None, 0, 3, 64, seed.ctypes.data_as(ctypes.c_void_p), ctypes.byref(h)) == 8
    assert b"null" in lib.dapol_last_error() and h.value == 0x1234
    assert lib.dapol_batch_store_create(None, None, 0, 3, 64, None, None) == 8
