"""dapol_compact_paths_plan / _expand / _compress through libdapol_hip.so: host-only exports (no context, no GPU), against the set model
of tests/test_compact_paths_cpu.py, with every refusal leaving its outputs untouched."""
import ctypes
import random

import numpy as np
import pytest

from test_compact_paths_cpu import model, random_indexes


def _cases():
    rng = random.Random(59)
    out = []
    for H in (1, 2, 6, 33, 64):
        top = (1 << H) - 1
        sets = [[], [0], [top], sorted({0, top})] + [random_indexes(rng, H, b) for b in ((2,) if H == 1 else (3, 4) if H == 2 else (9, 40))]
        if H == 6:
            sets.append(list(range(64)))
        out += [(H, s) for s in sets]
    return out


@pytest.mark.parametrize("leaf_first", [0, 1])
def test_plan_expand_compress_match_the_set_model(hip_lib, leaf_first):
    rng = np.random.default_rng(7)
    old = hip_lib.wire_config_set(siblings_leaf_first=leaf_first)
    try:
        for H, leaves in _cases():
            idx = np.array(leaves, np.uint64)
            b = len(leaves)
            _, depth_off, ref, _ = model(H, leaves)
            got_off, got_ref, n = hip_lib.compact_paths_plan(H, idx)
            assert got_off.tolist() == depth_off and n == depth_off[-1] and got_ref.tolist() == ref
            assert hip_lib.compact_paths_plan(H, idx, want_ref=False)[2] == n
            for hb in (32, 64):
                cC, cH = rng.integers(0, 256, size=(n, 32), dtype=np.uint8), rng.integers(0, 256, size=(n, hb), dtype=np.uint8)
                pC, pH = hip_lib.compact_paths_expand(H, idx, cC, cH, hash_bytes=hb)
                assert pC.shape == (b, H, 32) and pH.shape == (b, H, hb)
                for e in range(b):
                    for slot in range(H):
                        d = H - slot if leaf_first else slot + 1
                        rec = depth_off[d] + ref[d - 1][e]
                        assert pC[e, slot].tobytes() == cC[rec].tobytes() and pH[e, slot].tobytes() == cH[rec].tobytes()
                if b:
                    e = b // 2
                    oC, oH = hip_lib.compact_paths_expand(H, idx, cC, cH, first=e, count=1, hash_bytes=hb)             # one user's path
                    assert oC.tobytes() == pC[e].tobytes() and oH.tobytes() == pH[e].tobytes()
                zC, zH = hip_lib.compact_paths_compress(H, idx, pC, pH, hash_bytes=hb)
                assert zC.tobytes() == cC.tobytes() and zH.tobytes() == cH.tobytes()
                # compress does not read the rows behind a head: poison every slot at which the row is not one
                qC, qH = pC.copy(), pH.copy()
                for e in range(1, b):
                    for slot in range(H):
                        d = H - slot if leaf_first else slot + 1
                        if ref[d - 1][e] == ref[d - 1][e - 1]:
                            qC[e, slot], qH[e, slot] = 0xEE, 0xEE
                zC, zH = hip_lib.compact_paths_compress(H, idx, qC, qH, hash_bytes=hb)
                assert zC.tobytes() == cC.tobytes() and zH.tobytes() == cH.tobytes()
    finally:
        hip_lib.wire_config_restore(old)


def test_refusals_write_nothing(hip_lib):
    lib, p = hip_lib.lib(), (lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p))
    H, leaves = 6, [0, 1, 2, 3, 16, 17, 40, 63]
    idx = np.array(leaves, np.uint64)
    n = model(H, leaves)[1][-1]
    off, ref, cnt = np.full(H + 2, 0xAB, np.uint64), np.full((H, 8), 0xAB, np.uint32), ctypes.c_uint64(777)
    cC, cH = np.full((n + 2, 32), 0xAB, np.uint8), np.full((n + 2, 64), 0xAB, np.uint8)
    pC, pH = np.full((8, H, 32), 0xAB, np.uint8), np.full((8, H, 64), 0xAB, np.uint8)
    untouched = lambda *a: all((x == 0xAB).all() for x in a) and cnt.value == 777
    bad_sets = ([1, 0], [2, 2], [0, 64], [0, 16, 3])
    for bad in bad_sets:
        ix = np.array(bad, np.uint64)
        assert lib.dapol_compact_paths_plan(H, len(bad), p(ix), p(off), p(ref), ctypes.byref(cnt)) == 8 and untouched(off, ref)
        assert lib.dapol_compact_paths_expand(32, H, len(bad), p(ix), p(cC), p(cH), n, 0, len(bad), p(pC), p(pH)) == 8 and untouched(pC, pH)
        assert lib.dapol_compact_paths_compress(32, H, len(bad), p(ix), p(pC), p(pH), p(cC), p(cH), n + 2, ctypes.byref(cnt)) == 8 and untouched(cC, cH)
    assert lib.dapol_compact_paths_plan(65, 8, p(idx), p(off), p(ref), ctypes.byref(cnt)) == 1 and untouched(off, ref)
    assert lib.dapol_compact_paths_plan(0, 1, p(idx), p(off), p(ref), ctypes.byref(cnt)) == 8 and untouched(off, ref)
    for hb in (0, 16, 48, 33):
        assert lib.dapol_compact_paths_expand(hb, H, 8, p(idx), p(cC), p(cH), n, 0, 8, p(pC), p(pH)) == 8 and untouched(pC, pH)
        assert lib.dapol_compact_paths_compress(hb, H, 8, p(idx), p(pC), p(pH), p(cC), p(cH), n, ctypes.byref(cnt)) == 8 and untouched(cC, cH)
    for wrong in (n - 1, n + 1, 0):
        assert lib.dapol_compact_paths_expand(64, H, 8, p(idx), p(cC), p(cH), wrong, 0, 8, p(pC), p(pH)) == 8 and untouched(pC, pH)
    for first, count in ((0, 9), (8, 1), (9, 0), (3, 6)):
        assert lib.dapol_compact_paths_expand(64, H, 8, p(idx), p(cC), p(cH), n, first, count, p(pC), p(pH)) == 8 and untouched(pC, pH)
    for cap in (n - 1, 0):
        assert lib.dapol_compact_paths_compress(64, H, 8, p(idx), p(pC), p(pH), p(cC), p(cH), cap, ctypes.byref(cnt)) == 8 and untouched(cC, cH)
    assert b"cap_records" in lib.dapol_last_error()
    # every out pointer of the plan may be NULL; b = 0 is OK with no records
    assert lib.dapol_compact_paths_plan(H, 8, p(idx), None, None, None) == 0
    assert lib.dapol_compact_paths_plan(H, 0, None, None, None, ctypes.byref(cnt)) == 0 and cnt.value == 0
    cnt.value = 777
    assert lib.dapol_compact_paths_expand(32, H, 0, None, None, None, 0, 0, 0, None, None) == 0
    assert lib.dapol_compact_paths_compress(32, H, 0, None, None, None, None, None, 0, ctypes.byref(cnt)) == 0 and cnt.value == 0
    # exactly enough: the records, and nothing behind them
    assert lib.dapol_compact_paths_compress(64, H, 8, p(idx), p(pC), p(pH), p(cC), p(cH), n, ctypes.byref(cnt)) == 0 and cnt.value == n
    assert (cC[:n] == 0xAB).all() and (cC[n:] == 0xAB).all()                       # (the paths held 0xAB everywhere)
    cC[:n], cH[:n] = 0x11, 0x22
    assert lib.dapol_compact_paths_expand(64, H, 8, p(idx), p(cC), p(cH), n, 7, 1, p(pC), p(pH)) == 0
    assert (pC[0] == 0x11).all() and (pH[0] == 0x22).all()                         # count = 1: one row written
    assert (pC[1:] == 0xAB).all() and (pH[1:] == 0xAB).all()
