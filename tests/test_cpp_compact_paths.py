"""Dapol::generate_paths_compact / verify_proofs_compact_paths / CompactPaths::expand of include/dapol.hpp
(tests/cpp/dapol_hpp_compact_paths.cpp) compiled against libdapol_hip.so: the expansion equals the per-entity Merkle siblings, the
compact paths verify with as many merges as records, a non-canonical record fails exactly the proof whose path holds it."""
import os
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_cpp_compact_paths(hip_lib):
    hip_lib.lib()
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "dapol_hpp_compact_paths")
    libdir = os.path.join(ROOT, "dapol_amd")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "dapol_hpp_compact_paths.cpp"),
                    "-L", libdir, "-ldapol_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK compact paths n=40 records="), r.stdout + r.stderr
