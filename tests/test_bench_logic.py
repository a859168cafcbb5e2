"""bench.py's host logic that needs no GPU: which workload an (N, flags) pair names, the wall-budget planner, and the files
--dump-outputs writes."""
import argparse
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _args(**kw):
    d = dict(log2_entities=20, log2_entities_total=None, weak=False)
    d.update(kw)
    return argparse.Namespace(**d)


def test_default_workload_is_the_metrics_configuration_at_every_n():
    """BASELINE.json: "2^20 leaves, 1/2/4/8 GPU" -- the total stays 2^20 and N divides it (strong scaling); configs[3] is
    --log2-entities-total 22 on 8 GPUs; --weak keeps the per-GPU size instead."""
    assert bench.plan_workload(_args(), 1) == (1 << 20, 1 << 20, 20, "strong")       # the label of the series: N = 1, 2, 4, 8 agree
    for n in (2, 4, 8):
        assert bench.plan_workload(_args(), n) == (1 << 20, (1 << 20) // n, 20, "strong")
    assert bench.plan_workload(_args(log2_entities_total=22), 8) == (1 << 22, 1 << 19, 22, "strong")
    assert bench.plan_workload(_args(weak=True), 8) == (1 << 23, 1 << 20, 23, "weak")
    assert bench.plan_workload(_args(log2_entities=9, weak=True), 2) == (1024, 512, 10, "weak")
    with pytest.raises(SystemExit):
        bench.plan_workload(_args(), 3)
    with pytest.raises(SystemExit):
        bench.plan_workload(_args(log2_entities=1), 4)


def test_wall_budget_planner():
    # 19 s steps, 450 s left: the driver's 20 + 5 does not fit; timed steps come first, further warm-ups only out of slack
    extra, steps = bench.plan_steps(20, 5, 19.0, 450.0)
    assert steps == 20 and extra == 2
    extra, steps = bench.plan_steps(20, 5, 19.0, 300.0)
    assert steps == 15 and extra == 0
    assert bench.plan_steps(20, 5, 19.0, 10.0) == (0, 3)          # never fewer than three timed steps
    assert bench.plan_steps(3, 1, None, 100.0) == (0, 3)


def test_no_launcher_means_spawn_not_exit(monkeypatch):
    """`--gpus 2` with WORLD_SIZE unset goes to spawn_ranks (which starts torch.distributed.run as a CHILD); under a launcher the
    process is a rank."""
    called = {}
    monkeypatch.setattr(bench, "spawn_ranks", lambda a: called.setdefault("spawn", a.gpus))
    monkeypatch.setattr(bench, "mode_prove", lambda a: called.setdefault("prove", a.gpus))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    bench.main()
    assert called == {"spawn": 2}
    called.clear()
    monkeypatch.setenv("WORLD_SIZE", "2")
    bench.main()
    assert called == {"prove": 2}
    called.clear()
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    bench.main()
    assert called == {"prove": 1}


class _FakeProver:
    """What dump_outputs() reads of a ShardedProver after a step: the root, the sorted leaf indexes, paths and proofs by leaf."""

    def __init__(self, n, height, proof_size):
        self.height, self.proof_size, self.w = height, proof_size, object()
        self.idx = np.arange(n, dtype=np.uint64) * np.uint64(3)
        self.root = (bytes(range(32)), bytes(range(32, 64)), (1 << 40) + 5, bytes(range(64, 96)))

    def sample_paths(self, leaf_ids, pad_seed, with_nodes=False):
        b, h = len(leaf_ids), self.height
        sv = np.repeat(np.asarray(leaf_ids, np.uint64)[:, None], h, axis=1)
        tag = (np.asarray(leaf_ids) % 251).astype(np.uint8)[:, None, None]
        sr, sC, sH = (np.broadcast_to(tag + k, (b, h, 32)).copy() for k in (0, 1, 2))
        return (sv, sr, sC, sH) if with_nodes else (sv, sr)

    def sample_proofs(self, leaf_ids, proof_size):
        return np.repeat((np.asarray(leaf_ids) % 256).astype(np.uint8)[:, None], proof_size, axis=1)


def test_dump_outputs_sample_and_format(tmp_path):
    """--dump-outputs: float32 bytes (a u64 as its 8 little-endian bytes), every entity when they fit, a fixed seeded sample under
    64 MB at the headline shape (2^20 entities, height 32, 992-byte proofs), and the same files from run to run."""
    assert bench.dump_sample_size(1024, 16, 800) == 1024
    s = bench.dump_sample_size(1 << 20, 32, 992)
    assert 1000 < s < (1 << 20) and s * (4 * (992 + 32 * 104) + 8) + (64 << 10) <= bench.DUMP_MAX_BYTES

    small = bench.dump_outputs(str(tmp_path / "small"), _FakeProver(100, 8, 64), 0x0102030405060708, 64)
    assert small["entities"] == 100 and small["bytes"] <= bench.DUMP_MAX_BYTES
    load = lambda d, name: np.load(os.path.join(d, name + ".npy"))
    d = small["dir"]
    for name in small["files"]:
        assert load(d, name).dtype in (np.float32, np.float64), name
    assert load(d, "checksum").tolist() == [8, 7, 6, 5, 4, 3, 2, 1]
    assert load(d, "root_value").tolist() == [5, 0, 0, 0, 0, 1, 0, 0]
    assert load(d, "root_hash").tolist() == list(range(32, 64))
    assert load(d, "sample_positions").tolist() == list(range(100))
    assert load(d, "proofs").shape == (100, 64) and load(d, "path_hashes").shape == (100, 8, 32) and load(d, "path_values").shape == (100, 8, 8)
    assert load(d, "proofs")[7, 0] == 21 and load(d, "path_values")[7, 3].tolist() == [21, 0, 0, 0, 0, 0, 0, 0]

    big = [bench.dump_outputs(str(tmp_path / k), _FakeProver(1 << 20, 32, 992), 1, 992) for k in ("a", "b")]
    assert big[0]["entities"] == s and max(b["bytes"] for b in big) <= bench.DUMP_MAX_BYTES
    pos = load(big[0]["dir"], "sample_positions")
    assert len(np.unique(pos)) == s and np.all(np.diff(pos) > 0)
    for name in big[0]["files"]:
        assert np.array_equal(load(big[0]["dir"], name), load(big[1]["dir"], name)), name


def test_full_is_off_by_default_and_only_for_the_proving_workload(monkeypatch):
    """A plain run is the lean one; --full reaches mode_prove, and the modes that always run whole refuse it."""
    seen = []
    monkeypatch.setattr(bench, "mode_prove", lambda a: seen.append(a.full))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for argv, want in ((["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1"], False), (["bench.py", "--full"], True)):
        monkeypatch.setattr(sys, "argv", argv)
        bench.main()
        assert seen.pop() is want
    for extra in (["--mode", "build"], ["--mode", "verify"], ["--mode", "criterion"], ["--preflight"]):
        monkeypatch.setattr(sys, "argv", ["bench.py", "--full"] + extra)
        with pytest.raises(SystemExit, match="--full"):
            bench.main()
