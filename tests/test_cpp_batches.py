"""Dapol::generate_proof_batches / DapolBatchProof::verify_many of include/dapol.hpp (tests/cpp/dapol_hpp_batches.cpp) compiled against
libdapol_hip.so: the proofs of one call equal generate_proof_batch's, verify in one call, and a tampered, a misshapen and a foreign
proof are each rejected alone."""
import os
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_cpp_proof_batches_round_trip(hip_lib):
    hip_lib.lib()
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "dapol_hpp_batches")
    libdir = os.path.join(ROOT, "dapol_amd")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "dapol_hpp_batches.cpp"),
                    "-L", libdir, "-ldapol_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK batches n=8"), r.stdout + r.stderr
