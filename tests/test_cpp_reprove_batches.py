"""Dapol::regenerate_proof_batches of include/dapol.hpp (tests/cpp/dapol_hpp_reprove_batches.cpp) compiled against libdapol_hip.so."""
import os
import subprocess

import pytest

from conftest import ROOT


def _build(hip_lib):
    hip_lib.lib()
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "dapol_hpp_reprove_batches")
    libdir = os.path.join(ROOT, "dapol_amd")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "dapol_hpp_reprove_batches.cpp"),
                    "-L", libdir, "-ldapol_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    return exe


def test_cpp_reprove_batches_compiles_and_fails_loudly_without_gpu(hip_lib):
    exe = _build(hip_lib)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith(("NO_DEVICE", "OK reprove ")), r.stdout     # no device: says so; a device: the whole check ran


@pytest.mark.gpu
def test_cpp_reprove_batches_matches_the_batch_call_on_the_edited_tree(hip_lib):
    exe = _build(hip_lib)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK reprove batches=50 "), r.stdout + r.stderr
