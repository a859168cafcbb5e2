"""Dapol::generate_proofs_compact / verify_proofs_compact / CompactProofs::expand of include/dapol.hpp (tests/cpp/dapol_hpp_compact.cpp)
compiled against libdapol_hip.so: the expansion equals generate_proofs_shared's proofs, the compact form verifies with the plan's number
of range proofs, one flipped byte of a shared sub-proof fails exactly the proofs that use it."""
import os
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_cpp_compact_proofs(hip_lib):
    hip_lib.lib()
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "dapol_hpp_compact")
    libdir = os.path.join(ROOT, "dapol_amd")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "dapol_hpp_compact.cpp"),
                    "-L", libdir, "-ldapol_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK compact n=40 unique="), r.stdout + r.stderr
