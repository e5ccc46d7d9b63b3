"""bench.py's own plumbing: --dump-outputs writes the last timed step's factor stream (bounded, seeded
sample beyond the cap), a plain run leaves the side legs out and --full brings them back."""
from __future__ import annotations

import json
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, str(ROOT))
import bench  # noqa: E402


def test_dump_outputs_small_array_is_whole(tmp_path):
    F = np.array([[65, 0], [0, 3], [4000000000, 7]], np.uint32)
    assert bench.dump_outputs(tmp_path / "d", {"factors": F}) == {"factors": 3}
    G = np.load(tmp_path / "d" / "factors.npy")
    assert G.dtype == np.float64 and np.array_equal(G, F.astype(np.float64))


def test_dump_outputs_caps_with_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 1 << 12)
    a = np.arange(3000, dtype=np.uint64).reshape(1000, 3) * 3000000007  # 24 kB as float64, past 2^32
    b = np.arange(100, dtype=np.uint32)                                  # fits its share
    w1 = bench.dump_outputs(tmp_path / "r1", {"a": a, "b": b})
    w2 = bench.dump_outputs(tmp_path / "r2", {"a": a, "b": b})
    assert w1 == w2 == {"a": ((1 << 11) - bench.DUMP_HEADER_BYTES) // 24, "b": 100}
    A1, A2 = np.load(tmp_path / "r1" / "a.npy"), np.load(tmp_path / "r2" / "a.npy")
    assert np.array_equal(A1, A2) and A1.dtype == np.float64
    assert sum(p.stat().st_size for p in (tmp_path / "r1").glob("*.npy")) <= 1 << 12  # file bytes, headers included
    # every sampled row is a row of the input, each at most once, in ascending order
    rows = (A1[:, 0] / 3000000007 / 3).round().astype(np.int64)
    assert np.array_equal(A1, a[rows].astype(np.float64)) and np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(tmp_path / "r1" / "b.npy"), b.astype(np.float64))


def test_dump_outputs_default_cap_is_64_mb_of_file_bytes(tmp_path):
    """An output past the cap (a (4.2 M, 2) stream is 67 MB as float64): the file, header included, is
    within 64 * 10^6 bytes; a rank of two writes within half of that."""
    assert bench.DUMP_CAP_BYTES == 64 * 10**6
    F = np.arange(2 * 4200000, dtype=np.uint32).reshape(-1, 2)
    w = bench.dump_outputs(tmp_path / "w1", {"factors": F})
    size = (tmp_path / "w1" / "factors.npy").stat().st_size
    assert size <= 64 * 10**6 and w["factors"] == (64 * 10**6 - bench.DUMP_HEADER_BYTES) // 16
    bench.dump_outputs(tmp_path / "w2", {"factors_rank1": F}, bench.DUMP_CAP_BYTES // 2)
    assert (tmp_path / "w2" / "factors_rank1.npy").stat().st_size <= 32 * 10**6


def run_bench(*argv):
    """bench.py in a process of its own, as it is run: its stdout is one JSON result line."""
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), *argv], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


SMALL = ("--gpus", "1", "--size-mib", "2", "--steps", "3", "--warmup", "1")


@pytest.mark.gpu
def test_plain_run_dumps_the_oracle_stream(tmp_path, lz, orc):
    """The plain line keeps the headline fields, carries none of the side legs, and the dumped
    stream of the last timed step is the oracle's for the same (seeded) text."""
    d = run_bench(*SMALL, "--dump-outputs", str(tmp_path / "o1"))
    assert d["metric"] == "factorization MB/s (3-aprx LZ77, greedy + lpf_opt, tau=512)"
    assert (d["unit"], d["higher_is_better"], d["dtype"], d["steps"], d["warmup"]) == ("MB/s", True, "u8", 3, 1)
    assert d["ms_per_step"] > 0
    assert abs(d["value"] - (2 << 20) / (d["ms_per_step"] * 1e-3) / 1e6) <= 0.01 * d["value"]
    assert d["full"] is False and d["cpu_baseline"] is None
    cfg = d["config"]
    assert cfg["pcie_inclusive_mbps"] is None and cfg["device_decode"] is None and cfg["huffman_container"] is None
    F = np.load(tmp_path / "o1" / "factors.npy")
    assert F.dtype == np.float64 and F.shape == (cfg["factors"], 2) and d["dumped_outputs"] == {"factors": F.shape[0]}
    T = bench.make_text(lz, "rr", 2 << 20, 0)
    F_ref, _ = orc.factorize(T)
    assert np.array_equal(F, F_ref.astype(np.float64))


@pytest.mark.gpu
def test_full_run_keeps_the_side_legs():
    d = run_bench(*SMALL, "--full")
    assert d["full"] is True and d["dumped_outputs"] is None
    cfg = d["config"]
    assert cfg["device_decode"]["mismatches"] == 0
    assert cfg["huffman_container"]["bytes"] > 0 and cfg["pcie_inclusive_mbps"] > 0
    cpu = d["cpu_baseline"]
    assert cpu["unit"] == "MB/s" and cpu["value"] > 0 and cpu["p1"]["factors"] == cfg["factors"]
