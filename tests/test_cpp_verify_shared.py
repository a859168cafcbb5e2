"""Dapol::verify_proofs_shared of include/dapol.hpp (tests/cpp/dapol_hpp_verify_shared.cpp) compiled against libdapol_hip.so:
generate_proofs_shared -> verify_proofs_shared -> all true with fewer range proofs checked than sub-proofs; one tampered copy of a
shared sub-proof -> exactly that proof false."""
import os
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_cpp_verify_proofs_shared(hip_lib):
    hip_lib.lib()
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "dapol_hpp_verify_shared")
    libdir = os.path.join(ROOT, "dapol_amd")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "dapol_hpp_verify_shared.cpp"),
                    "-L", libdir, "-ldapol_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK verify_shared n=40 unique="), r.stdout + r.stderr
