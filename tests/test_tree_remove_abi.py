"""dapol_tree_remove in the C ABI, without a device: declared, exported and bound; argument checks come before any device work."""
import ctypes

import numpy as np

from test_abi import declared_symbols


def test_remove_is_declared_exported_and_bound(hip_lib):
    assert "dapol_tree_remove" in declared_symbols()
    assert hasattr(hip_lib.lib(), "dapol_tree_remove")
    assert "dapol_tree_remove" in hip_lib.EXPORTED_SYMBOLS
    assert callable(getattr(hip_lib.Tree, "remove", None))


def test_remove_without_a_tree_is_an_invalid_argument(hip_lib):
    lib = hip_lib.lib()
    idx = np.array([5], np.uint64)
    assert lib.dapol_tree_remove(None, 1, idx.ctypes.data_as(ctypes.c_void_p)) == 8
    assert lib.dapol_tree_remove(None, 0, None) == 8
    assert b"null" in lib.dapol_last_error()
