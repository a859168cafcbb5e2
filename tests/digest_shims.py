"""What the SHA-256 / SHA3-256 tests share: the two hashlib digests registered with the Python oracle, the host build
(tests/digest_host_shim.cpp) and the gfx950 build (tests/digest_dev_shim.hip) of the cases in tests/digest_cases.h, and their inputs."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
CSRC = os.path.join(ROOT, "dapol_amd", "csrc")
BUILD = os.path.join(TESTS, "_build")

# name in pyref.DIGESTS -> (DAPOL_DIGEST_* id, hashlib constructor)
NEW_DIGESTS = {"sha256": (4, hashlib.sha256), "sha3_256": (5, hashlib.sha3_256)}
STREAM_LENGTHS = list(range(301)) + [1000, 5000]      # crosses SHA-256's padding edges (55, 56, 63, 64, 65, 119, 120) and SHA-3's (135 .. 137, 271 .. 273)
PIECES = (0, 1, 7, 64)                                # 0: the whole message in one call
DEV_LANES = 300                                       # lane L of the device launch hashes the L-byte counter pattern
_SOURCES = [os.path.join(TESTS, "digest_cases.h")] + [os.path.join(CSRC, f) for f in ("hash.h", "fe.h", "labels.h")]


def register(pyref):
    """OpenSSL's SHA-2 and SHA-3 become the oracle's digests "sha256" and "sha3_256" (pyref.DIGESTS is a plain dict keyed by name)."""
    for name, (_, ctor) in NEW_DIGESTS.items():
        pyref.DIGESTS.setdefault(name, (ctor, 32))


def counter(n):
    return bytes(i & 255 for i in range(n))


def node_inputs():
    """64 random inputs of 128 bytes, all zero, all 0xFF -> uint32 [66][32]"""
    rnd = np.random.default_rng(256).integers(0, 1 << 32, size=(64, 32), dtype=np.uint64).astype(np.uint32)
    return np.ascontiguousarray(np.concatenate([rnd, np.zeros((1, 32), np.uint32), np.full((1, 32), 0xFFFFFFFF, np.uint32)]))


def _stale(target, sources):
    stamp = target + ".sources"
    h = hashlib.sha256()
    for s in sources:
        with open(s, "rb") as f:
            h.update(f.read())
    return not (os.path.exists(target) and os.path.exists(stamp) and open(stamp).read() == h.hexdigest()), stamp, h.hexdigest()


def _build(target, sources, cmd):
    os.makedirs(BUILD, exist_ok=True)
    stale, stamp, digest = _stale(target, sources)
    if stale:
        subprocess.run(cmd, check=True, cwd=TESTS)
        with open(stamp, "w") as f:
            f.write(digest)
    return target


def build_host_shim():
    so = os.path.join(BUILD, "digest_host_shim.so")
    src = os.path.join(TESTS, "digest_host_shim.cpp")
    return _build(so, [src] + _SOURCES, ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", so])


def build_dev_shim():
    """-> tests/_build/digest_dev_shim.so with the library's own flags (cross-compiles without a device)"""
    so = os.path.join(BUILD, "digest_dev_shim.so")
    src = os.path.join(TESTS, "digest_dev_shim.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return _build(so, [src] + _SOURCES, [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", src, "-o", so])


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Cases:
    """prefix "t_": the host shim (void functions); "d_": the device shim (every function returns a hipError_t, which must be 0)."""

    def __init__(self, lib, prefix):
        self.lib, self.prefix = lib, prefix

    def _call(self, name, *args):
        fn = getattr(self.lib, self.prefix + name)
        fn.restype = ctypes.c_int if self.prefix == "d_" else None
        rc = fn(*args)
        assert self.prefix != "d_" or rc == 0, "%s%s returned hipError_t %d" % (self.prefix, name, rc)

    def stream(self, kind, msg, piece):
        """host only -> the digest's 32 bytes"""
        out = np.zeros(8, np.uint32)
        self._call("digest_stream", kind, msg, ctypes.c_size_t(len(msg)), ctypes.c_size_t(piece), _p(out))
        return out.astype("<u4").tobytes()

    def stream_cases(self, kind, n):
        """-> uint32 [n][8]: row L = the digest of the L-byte counter pattern"""
        out = np.zeros((n, 8), np.uint32)
        self._call("digest_stream_cases", kind, n, _p(out))
        return out

    def node_cases(self, kind, inputs):
        """-> (D(in[..32]), D(in[..128])) as uint32 [n][8] each"""
        n = len(inputs)
        a, b = np.zeros((n, 8), np.uint32), np.zeros((n, 8), np.uint32)
        self._call("digest_node_cases", kind, n, _p(inputs), _p(a), _p(b))
        return a, b


def host_cases():
    return Cases(ctypes.CDLL(build_host_shim()), "t_")


def dev_cases():
    return Cases(ctypes.CDLL(build_dev_shim()), "d_")
