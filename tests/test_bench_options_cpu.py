"""bench.py's command line (no GPU): a plain run is the headline's timed steps
alone, every other leg sits behind --full, and --dump-outputs writes the last
timed pass's results as float64 arrays of a bounded size."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_not_full(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (a.full, a.steps, a.warmup, a.dump_outputs) == (False, 7, 3, None)
    assert _parse(monkeypatch, "--full").full


@pytest.mark.parametrize("argv", [("--only", "score"), ("--only", "C5"), ("--c4",)])
def test_leg_selectors_need_full(monkeypatch, argv):
    with pytest.raises(SystemExit) as e:
        _parse(monkeypatch, *argv)
    assert e.value.code == 2
    assert _parse(monkeypatch, "--full", *argv).full


def test_dump_outputs_needs_the_placement_leg(monkeypatch, tmp_path):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--full", "--only", "vote", "--dump-outputs", str(tmp_path))
    a = _parse(monkeypatch, "--full", "--only", "place", "--dump-outputs", str(tmp_path))
    assert a.dump_outputs == str(tmp_path)


def test_dump_outputs_writes_float64_arrays(tmp_path):
    node = np.array([3, -1, 0, 9999], np.int32)
    score = np.array([2**40 + 1, 0, -5, 7], np.int64)
    info = bench.dump_outputs(str(tmp_path / "d"), {"node": node, "score": score})
    got_n, got_s = np.load(tmp_path / "d" / "node.npy"), np.load(tmp_path / "d" / "score.npy")
    assert got_n.dtype == got_s.dtype == np.float64
    assert got_n.tolist() == node.tolist() and got_s.tolist() == score.tolist()
    assert info["pods"] == 4 and info["sample"] is None


def test_dump_outputs_samples_above_the_size_limit(tmp_path):
    n = 1000
    last = {"node": np.arange(n, dtype=np.int32), "score": np.arange(n, dtype=np.int64) * 3}
    sizes = []
    for sub in ("a", "b"):  # the same seeded sample every time, aligned across the arrays
        info = bench.dump_outputs(str(tmp_path / sub), last, limit_bytes=16 * 100)
        assert info["pods"] == 100
        sizes.append((np.load(tmp_path / sub / "node.npy"), np.load(tmp_path / sub / "score.npy")))
    (n0, s0), (n1, s1) = sizes
    assert len(n0) == 100 and n0.nbytes + s0.nbytes <= 16 * 100
    assert (np.diff(n0) > 0).all() and (s0 == 3 * n0).all()
    assert (n0 == n1).all() and (s0 == s1).all()
