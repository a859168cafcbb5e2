"""dapol_tree_insert in the C ABI, without a device: declared, exported and bound in every layer; argument checks come before any
device work; the host plan of its general path exists."""
import ctypes
import os

import numpy as np

from conftest import ROOT
from test_abi import declared_symbols


def test_insert_is_declared_exported_and_bound(hip_lib):
    assert "dapol_tree_insert" in declared_symbols()
    assert hasattr(hip_lib.lib(), "dapol_tree_insert")
    assert "dapol_tree_insert" in hip_lib.EXPORTED_SYMBOLS
    assert callable(getattr(hip_lib.Tree, "insert", None))
    assert "5" in hip_lib.Tree.last_update_path.__doc__


def test_the_cpp_wrapper_and_the_host_plan_exist():
    hpp = open(os.path.join(ROOT, "include", "dapol.hpp")).read()
    assert "void insert(const std::vector<uint64_t>& idx" in hpp and "dapol_tree_insert(" in hpp
    assert "plan_insert_general(" in open(os.path.join(ROOT, "dapol_amd", "csrc", "tree_edit_plan.inc")).read()


def test_insert_argument_checks_need_no_device(hip_lib):
    lib = hip_lib.lib()
    idx, v, r = np.array([5], np.uint64), np.array([1], np.uint64), np.zeros(32, np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.dapol_tree_insert(None, 1, p(idx), p(v), p(r)) == 8
    assert b"null" in lib.dapol_last_error()
    assert lib.dapol_tree_insert(None, 0, None, None, None) == 8
