"""Dapol::batch_store / BatchProofStore of include/dapol.hpp (tests/cpp/dapol_hpp_batch_store.cpp) compiled against libdapol_hip.so."""
import os
import subprocess

import pytest

from conftest import ROOT


def _build(hip_lib):
    hip_lib.lib()
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "dapol_hpp_batch_store")
    libdir = os.path.join(ROOT, "dapol_amd")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "dapol_hpp_batch_store.cpp"),
                    "-L", libdir, "-ldapol_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    return exe


def test_cpp_batch_store_compiles_and_fails_loudly_without_gpu(hip_lib):
    exe = _build(hip_lib)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith(("NO_DEVICE", "OK batch_store ")), r.stdout       # no device: says so; a device: the whole check ran


@pytest.mark.gpu
def test_cpp_batch_store_serves_the_batch_reprovers_proofs(hip_lib):
    exe = _build(hip_lib)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK batch_store batches=21 "), r.stdout + r.stderr
