"""numpy front end of the raw-limb case runners: tests/host_shim.cpp (t_*_cases, the host path) and tests/dev_shim.hip
(d_*_cases, the device path) take the same arguments, so one class serves both and the tests can hold the two side by side."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
CSRC = os.path.join(ROOT, "dapol_amd", "csrc")

# tests/arith_cases.h
FE_MUL, FE_SQ, FE_CARRY, FE_ADDC, FE_TOWORDS, FE_ABS, FE_INVERT, FE_POW22523, FE_SQRT_RATIO = range(9)
GE_MADD, GE_ADD, GE_DBL, GE_ADD_CACHED, GE_NEG, GE_CHAIN = range(6)
SC_MUL, SC_ADD, SC_SUB, SC_INVERT, SC_INVERT_VARTIME, SC_FROM_U64, SC_MONTMUL_RAW = range(7)
GE_CHAIN_ROUNDS, GE_CHAIN_DBLS, RECODE_MAX_NW = 4, 8, 32

DEV_SOURCES = [os.path.join(TESTS, f) for f in ("dev_shim.hip", "arith_cases.h")] + \
              [os.path.join(CSRC, f) for f in ("fe.h", "ge.h", "ge_quad.h", "tables.h", "sc.h", "hash.h", "consts.h", "labels.h")]


def build_dev_shim():
    """tests/dev_shim.hip -> tests/_build/dev_shim.so with the library's own flags (cross-compiles without a device).  Rebuilt
    when the CONTENT of a source differs from what the existing file was built from."""
    out = os.path.join(TESTS, "_build")
    os.makedirs(out, exist_ok=True)
    so, stamp = os.path.join(out, "dev_shim.so"), os.path.join(out, "dev_shim.so.sources")
    h = hashlib.sha256()
    for s in DEV_SOURCES:
        with open(s, "rb") as f:
            h.update(f.read())
    if os.path.exists(so) and os.path.exists(stamp) and open(stamp).read() == h.hexdigest():
        return so
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", DEV_SOURCES[0], "-o", so], check=True, cwd=TESTS)
    with open(stamp, "w") as f:
        f.write(h.hexdigest())
    return so


def _i32(a, width):
    a = np.ascontiguousarray(np.array(a, dtype=np.int64).reshape(-1, width), dtype=np.int32)
    return a


def _u32_of_ints(xs, nwords):
    return np.array([[(int(x) >> (32 * i)) & 0xFFFFFFFF for i in range(nwords)] for x in xs], dtype=np.uint32).reshape(-1, nwords)


def _u32_of_bytes(bs, nwords):
    return np.frombuffer(b"".join(bs), dtype="<u4").reshape(-1, nwords).copy()


def ints_of_words(w):
    return [sum(int(v) << (32 * i) for i, v in enumerate(row)) for row in w]


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Cases:
    """prefix "t_": host_shim.so (void functions); prefix "d_": dev_shim.so (every function returns a hipError_t, which must
    be 0 -- a wrapper that saw an error is a failed test, whatever it copied back)."""

    def __init__(self, lib, prefix):
        self.lib, self.prefix, self.checked = lib, prefix, prefix == "d_"

    def _call(self, name, *args):
        fn = getattr(self.lib, self.prefix + name)
        fn.restype = ctypes.c_int if self.checked else None
        rc = fn(*args)
        if self.checked:
            assert rc == 0, "%s%s returned hipError_t %d" % (self.prefix, name, rc)

    def fe(self, op, F, G=None):
        """-> (limbs [n][9] int32, values of the canonical words [n], flags [n])"""
        F = _i32(F, 9)
        G = _i32(G, 9) if G is not None else np.zeros_like(F)
        n = len(F)
        assert len(G) == n
        ol, ow, fl = np.zeros((n, 9), np.int32), np.zeros((n, 8), np.uint32), np.zeros(n, np.int32)
        self._call("fe_cases", op, n, _p(F), _p(G), _p(ol), _p(ow), _p(fl))
        return ol, ints_of_words(ow), fl

    def ge(self, op, Pl, Ql, neg, quad=False):
        """-> (limbs [n][36], encodings [n] as bytes) -- the quad runner returns the limbs alone"""
        Pl, Ql = _i32(Pl, 36), _i32(Ql, 36)
        n = len(Pl)
        neg = np.ascontiguousarray(np.array(neg, dtype=np.int32))
        assert len(Ql) == n and len(neg) == n
        ol, ow = np.zeros((n, 36), np.int32), np.zeros((n, 8), np.uint32)
        if quad:
            self._call("quad_cases", op, n, _p(Pl), _p(Ql), _p(neg), _p(ol))
            return ol
        self._call("ge_cases", op, n, _p(Pl), _p(Ql), _p(neg), _p(ol), _p(ow))
        return ol, [row.astype("<u4").tobytes() for row in ow]

    def decompress(self, encs):
        w = _u32_of_bytes(encs, 8)
        n = len(w)
        ok, ol, ow = np.zeros(n, np.int32), np.zeros((n, 36), np.int32), np.zeros((n, 8), np.uint32)
        self._call("ge_decompress_cases", n, _p(w), _p(ok), _p(ol), _p(ow))
        return ok, ol, [row.astype("<u4").tobytes() for row in ow]

    def uniform(self, b64s):
        w = _u32_of_bytes(b64s, 16)
        n = len(w)
        ol, ow = np.zeros((n, 36), np.int32), np.zeros((n, 8), np.uint32)
        self._call("ge_uniform_cases", n, _p(w), _p(ol), _p(ow))
        return ol, [row.astype("<u4").tobytes() for row in ow]

    def sc(self, op, a, b):
        A, B = _u32_of_ints(a, 8), _u32_of_ints(b, 8)
        out = np.zeros((len(A), 8), np.uint32)
        self._call("sc_cases", op, len(A), _p(A), _p(B), _p(out))
        return ints_of_words(out)

    def sc_wide(self, b64s):
        w = _u32_of_bytes(b64s, 16)
        out = np.zeros((len(w), 8), np.uint32)
        self._call("sc_wide_cases", len(w), _p(w), _p(out))
        return ints_of_words(out)

    def recode(self, cases):
        """cases: [(W, NW, x, ...)] -> [digits]"""
        wn = np.array([[c[0], c[1]] for c in cases], dtype=np.int32)
        x = _u32_of_ints([c[2] for c in cases], 8)
        d = np.zeros((len(cases), RECODE_MAX_NW), np.int32)
        self._call("sc_recode_cases", len(cases), _p(wn), _p(x), _p(d))
        return [[int(v) for v in d[i, :cases[i][1]]] for i in range(len(cases))]

    def strobe(self, kn, filler, words, words_rev):
        """device only.  -> (out [ncase][2][32] uint32, pos [ncase][2])"""
        kn = np.ascontiguousarray(np.array(kn, dtype=np.int32).reshape(-1, 2))
        w, wr = np.ascontiguousarray(words, dtype=np.uint32), np.ascontiguousarray(words_rev, dtype=np.uint32)
        out, pos = np.zeros((len(kn), 2, 32), np.uint32), np.zeros((len(kn), 2), np.uint32)
        self._call("strobe_cases", len(kn), _p(kn), filler, len(filler), _p(w), _p(wr), len(w), _p(out), _p(pos))
        return out, pos
