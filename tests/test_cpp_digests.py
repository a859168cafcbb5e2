"""include/dapol.hpp with DAPOL_DIGEST_SHA256 / DAPOL_DIGEST_SHA3_256 (tests/cpp/dapol_hpp_digests.cpp) compiled against libdapol_hip.so."""
import os
import subprocess

import pytest

from conftest import ROOT


def _build(hip_lib):
    hip_lib.lib()
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "dapol_hpp_digests")
    libdir = os.path.join(ROOT, "dapol_amd")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "dapol_hpp_digests.cpp"),
                    "-L", libdir, "-ldapol_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    return exe


def test_cpp_digests_compile_and_refuse_without_gpu(hip_lib):
    """ids 3, 6, -1 (and the 64-byte Blake2b) throw before the library is called; only then does the program look for a device"""
    exe = _build(hip_lib)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith(("NO_DEVICE", "OK digests 4 5")), r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_create_under_sha256_and_sha3_256(hip_lib):
    exe = _build(hip_lib)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK digests 4 5"), r.stdout + r.stderr
