"""dapol_tree_apply at the C ABI, as far as it goes without a device: the symbol is declared, exported and bound with eight arguments,
null arguments are refused before anything else is looked at, and the header documents the order in which the rules are checked.
(Everything past the argument check needs a tree, which needs a GPU: tests/test_gpu_tree_apply.py.)"""
import ctypes
import os
import re

import numpy as np

from conftest import ROOT


def _header():
    return open(os.path.join(ROOT, "include", "dapol_hip.h")).read()


def test_symbol_is_declared_exported_and_bound(hip_lib):
    lib = hip_lib.lib()
    assert "dapol_tree_apply" in hip_lib.EXPORTED_SYMBOLS and hasattr(lib, "dapol_tree_apply")
    decl = re.search(r"int32_t dapol_tree_apply\((.*?)\);", _header(), flags=re.S).group(1)
    params = [p.strip() for p in decl.split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == ["tree", "n_remove", "remove_idx", "n_put", "put_idx", "put_v", "put_r32", "put_was_new"]
    assert len(lib.dapol_tree_apply.argtypes) == len(params) and lib.dapol_tree_apply.restype is ctypes.c_int32
    assert [a is ctypes.c_size_t for a in lib.dapol_tree_apply.argtypes] == [p.startswith("size_t") for p in params]


def test_null_arguments_and_empty_batches(hip_lib):
    lib = hip_lib.lib()
    idx = np.array([1, 2], np.uint64)
    v = np.array([5, 6], np.uint64)
    r = np.zeros((2, 32), np.uint8)
    was = np.zeros(2, np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    # no tree: refused whatever else is passed, also an empty batch (as dapol_tree_update refuses it)
    for args in ((0, None, 0, None, None, None, None), (2, p(idx), 2, p(idx), p(v), p(r), p(was)), (1, p(idx), 0, None, None, None, None)):
        assert lib.dapol_tree_apply(None, *args) == 8
        assert b"null argument" in lib.dapol_last_error()
    assert lib.dapol_tree_update(None, 0, None, None, None) == 8
    assert not was.any()                                              # put_was_new is written on success only
    # a count with no array behind it is a null argument too: checked before the tree is looked at, so a tree handle that is never
    # dereferenced serves here
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(4096)))
    for args in ((1, None, 0, None, None, None, None), (0, None, 1, None, p(v), p(r), None), (0, None, 1, p(idx), None, p(r), None),
                 (0, None, 1, p(idx), p(v), None, None), (1, None, 1, p(idx), p(v), p(r), p(was))):
        assert lib.dapol_tree_apply(fake, *args) == 8
        assert b"null argument" in lib.dapol_last_error()
    # nothing to do is no error and looks at nothing: not at the tree, not at stale pointers (put_was_new may be NULL or not)
    assert lib.dapol_tree_apply(fake, 0, None, 0, None, None, None, None) == 0
    assert lib.dapol_tree_apply(fake, 0, p(idx), 0, p(idx), p(v), p(r), p(was)) == 0 and not was.any()


def test_the_header_states_the_order_of_the_rules():
    """The validation order is part of the contract (a batch that breaks two rules reports the first): the host's own rules -- an index
    twice among the puts, an index both removed and put -- then a removal that is not a leaf, then a put out of range / an empty result."""
    doc = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int32_t dapol_tree_apply\(", _header(), flags=re.S).group(1)
    order = [doc.index(s) for s in ("twice in put_idx", "both remove_idx and put_idx", "not a leaf", "outside the tree or outside a shard's prefix -> the code", "no leaf left")]
    assert order == sorted(order) and "in this order" in doc
    assert "6 = applied in place by dapol_tree_apply" in _header().replace("\n * ", " ")
