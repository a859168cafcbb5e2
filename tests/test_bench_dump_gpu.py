"""bench.py --dump-outputs on the GPU: exactly --steps timed steps, and the arrays dumped after them are the C oracle's bytes for
the same seeded inputs -- the tree root, every entity's inclusion path and a sample of the range proofs."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


@pytest.mark.gpu
def test_bench_dump_outputs_are_the_oracles_bytes(hip_lib, ref, tmp_path):
    height, n_bits, n = 16, 64, 1024
    out = str(tmp_path / "dump")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--log2-entities", "10", "--height", str(height), "--steps", "2", "--warmup", "1",
           "--no-cpu-baseline", "--no-secondary", "--dump-outputs", out]
    run = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, DAPOL_TABLE_GB="3"), capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-2000:]
    line = json.loads([l for l in run.stdout.splitlines() if l.startswith("{")][-1])
    assert line["complete"] and line["steps"] == 2 and line["ms_per_step"] > 0
    d = line["outputs_dumped"]
    assert d["dir"] == out and d["entities"] == d["entities_of_rank"] == n and d["bytes"] <= bench.DUMP_MAX_BYTES
    assert sorted(os.listdir(out)) == sorted(f + ".npy" for f in d["files"])
    got = {f: np.load(os.path.join(out, f + ".npy")) for f in d["files"]}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    b = {f: a.astype(np.uint8) for f, a in got.items() if f != "sample_positions"}
    assert got["sample_positions"].tolist() == list(range(n))
    assert "%016x" % int.from_bytes(b["checksum"].tobytes(), "little") == line["checksum"]

    idx, v, r = bench.synth_inputs(n, height, 0, n, n_bits)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    t = ctypes.c_void_p(ref.ref_tree_build(height, ctypes.c_size_t(n), p(idx), p(v), p(r), bench.PAD_SEED, 0))
    try:
        oC, oH, orr, ov = [ctypes.create_string_buffer(32) for _ in range(3)] + [ctypes.c_uint64()]
        ref.ref_tree_root(t, oC, oH, ctypes.byref(ov), orr)
        assert (b["root_commitment"].tobytes(), b["root_hash"].tobytes(), b["root_blinding"].tobytes()) == (oC.raw, oH.raw, orr.raw)
        assert int.from_bytes(b["root_value"].tobytes(), "little") == ov.value == int(v.sum())
        for k in range(n):
            sC, sH, sr = [ctypes.create_string_buffer(32 * height) for _ in range(3)]
            sv = np.zeros(height, np.uint64)
            assert ref.ref_tree_path(t, ctypes.c_uint64(int(idx[k])), sC, sH, p(sv), sr) == 1
            assert (b["path_commitments"][k].tobytes(), b["path_hashes"][k].tobytes(), b["path_blindings"][k].tobytes()) == (sC.raw, sH.raw, sr.raw)
            assert b["path_values"][k].tobytes() == sv.astype("<u8").tobytes()
        ps = b["proofs"].shape[1]
        sample = np.ascontiguousarray(idx[::64])
        proofs = ctypes.create_string_buffer(ps * len(sample))
        assert ref.ref_prove_entities_padding(t, ctypes.c_size_t(len(sample)), p(sample), n_bits, bench.NONCE_SEED, 0, proofs) == 0
        assert b["proofs"][::64].tobytes() == proofs.raw
    finally:
        ref.ref_tree_free(t)
