"""SHA-256 and SHA3-256 (DAPOL_DIGEST_SHA256 / DAPOL_DIGEST_SHA3_256) without a GPU: dapol_amd/csrc/hash.h compiled for the host against
hashlib (OpenSSL), the same under AddressSanitizer + UBSan as a stand-alone program, the Python oracle's known answers under the two
hashlib digests, and the cross-compilation of the device program that tests/test_digests_gpu.py runs."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import digest_shims as S
from conftest import ROOT

KAT_LIABILITIES = [(b"a", b"w", 3), (b"b", b"x", 5), (b"c", b"y", 7), (b"d", b"z", 11)]   # src/dapol/tests.rs:30-85 (values: tests/golden/kat.json)
KAT_INDEX = {"sha256": {b"a": 8, b"b": 15, b"c": 9, b"d": 2}, "sha3_256": {b"a": 2, b"b": 15, b"c": 1, b"d": 4}}


@pytest.fixture(scope="module")
def host():
    return S.host_cases()


@pytest.mark.parametrize("name", sorted(S.NEW_DIGESTS))
def test_host_streaming_digest_equals_hashlib(host, name):
    """Every length 0 .. 300, 1,000 and 5,000 of the counter pattern, in one call and in pieces of 1, 7 and 64 bytes."""
    kind, ctor = S.NEW_DIGESTS[name]
    for n in S.STREAM_LENGTHS:
        msg, want = S.counter(n), ctor(S.counter(n)).digest()
        for piece in S.PIECES:
            assert host.stream(kind, msg, piece) == want, (n, piece)
    got = host.stream_cases(kind, S.DEV_LANES)                 # the device launch's cases (byte by byte), for the GPU test to compare words with
    assert [row.astype("<u4").tobytes() for row in got] == [ctor(S.counter(n)).digest() for n in range(S.DEV_LANES)]


@pytest.mark.parametrize("name", sorted(S.NEW_DIGESTS))
def test_host_node_hashes_equal_hashlib(host, name):
    """leaf = D(C), 32 bytes; parent = D(C_L || C_R || H_L || H_R), 128 bytes: 64 random inputs, all zero, all 0xFF."""
    kind, ctor = S.NEW_DIGESTS[name]
    inputs = S.node_inputs()
    h32, h128 = host.node_cases(kind, inputs)
    for i, row in enumerate(inputs):
        b = row.astype("<u4").tobytes()
        assert h32[i].astype("<u4").tobytes() == ctor(b[:32]).digest(), i
        assert h128[i].astype("<u4").tobytes() == ctor(b).digest(), i


def test_digests_under_asan_and_ubsan():
    """tests/cpp/digest_asan.cpp: the two tests above as a stand-alone program built with the sanitizers, run as a child process; the
    expected digests come from hashlib through a file."""
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe, vec = os.path.join(out, "digest_asan"), os.path.join(out, "digest_asan_vectors.bin")
    inputs = S.node_inputs()
    with open(vec, "wb") as f:
        f.write(struct.pack("<I", len(S.STREAM_LENGTHS)) + np.array(S.STREAM_LENGTHS, "<u4").tobytes())
        for n in S.STREAM_LENGTHS:
            for name in ("sha256", "sha3_256"):
                f.write(S.NEW_DIGESTS[name][1](S.counter(n)).digest())
        f.write(struct.pack("<I", len(inputs)) + inputs.astype("<u4").tobytes())
        for row in inputs:
            b = row.astype("<u4").tobytes()
            for part in (b[:32], b):
                for name in ("sha256", "sha3_256"):
                    f.write(S.NEW_DIGESTS[name][1](part).digest())
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    os.path.join(ROOT, "tests", "cpp", "digest_asan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, vec], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "digest asan clean" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


def test_oracle_known_answers_under_the_hashlib_digests(pyref):
    """The reference's KAT liabilities (ids a, b, c, d; external w, x, y, z; seed "test"; height 4) through pyref.dapol_new with
    hashlib's SHA-256 and SHA3-256 registered: the indexes below and the root value 26.  Blake2s gives the reference's own
    7, 12, 2, 4 (src/dapol/tests.rs:30-85) through the same call.  This pins the oracle the GPU tests compare against."""
    S.register(pyref)
    for name, want in KAT_INDEX.items():
        assert pyref.DIGESTS[name] == (S.NEW_DIGESTS[name][1], 32)
        tree, id_map = pyref.dapol_new(KAT_LIABILITIES, b"test", 4, bytes(32), name)
        assert id_map == want and tree.root.v == 26, name
    _, id_map = pyref.dapol_new(KAT_LIABILITIES, b"test", 4, bytes(32), "blake2s")
    assert id_map == {b"a": 7, b"b": 12, b"c": 2, b"d": 4}


def test_digest_device_program_cross_compiles():
    """no device needed: hipcc builds tests/digest_dev_shim.hip for gfx950 with the library's flags, and the wrappers are there"""
    lib = ctypes.CDLL(S.build_dev_shim())
    for name in ("digest_stream_cases", "digest_node_cases"):
        assert hasattr(lib, "d_" + name)
