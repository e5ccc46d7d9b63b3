"""CPU tests of the range extract: the host form (lz77sss_extract_u32 / _u64) against slices of the
host decode, and the argument checks of the device forms, which come before the device is touched."""
from __future__ import annotations

import ctypes
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden_names, load_golden
from decode_streams import chain_stream, invalid_streams, period3_stream, random_streams, run_stream

NEW_SYMBOLS = ["lz77sss_session_decode_windowed", "lz77sss_session_extract", "lz77sss_decode_u32_device_windowed",
               "lz77sss_decode_u64_device_windowed", "lz77sss_extract_u32_device", "lz77sss_extract_u64_device",
               "lz77sss_extract_u32", "lz77sss_extract_u64"]


def ranges(n, seed):
    R = [(0, 0), (0, n), (n, 0)]
    if n:
        R += [(0, 1), (n - 1, 1), (n // 2, n - n // 2)]
    rng = np.random.default_rng(seed)
    for _ in range(16 if n else 0):
        p = int(rng.integers(0, n))
        R.append((p, int(rng.integers(0, n - p + 1))))
    return R


def test_new_symbols_exported(lz):
    lib = ctypes.CDLL(str(lz.LIB_PATH))
    header = (ROOT / "include" / "lz77sss.h").read_text()
    for sym in NEW_SYMBOLS:
        assert hasattr(lib, sym) and sym in lz._SYMBOLS and sym + "(" in header, sym
    for fn in ("decode_device_windowed", "extract_device", "extract"):
        assert callable(getattr(lz, fn))
    for fn in ("decode_windowed", "extract"):
        assert callable(getattr(lz.Session, fn))


@pytest.mark.parametrize("name", golden_names())
def test_extract_golden(lz, name):
    g = load_golden(name)
    T, F = g["text"], g["factors"]
    for pos, ln in ranges(T.size, 7):
        assert np.array_equal(lz.extract(F, T.size, pos, ln), T[pos:pos + ln]), (pos, ln)
    F64 = F.astype(np.uint64)
    for pos, ln in ranges(T.size, 8)[:8]:
        assert np.array_equal(lz.extract(F64, T.size, pos, ln), T[pos:pos + ln]), (pos, ln)


def test_extract_random_streams(lz):
    for F, n in random_streams():
        T = lz.decode(F, n)
        for pos, ln in ranges(n, n):
            assert np.array_equal(lz.extract(F, n, pos, ln), T[pos:pos + ln]), (n, pos, ln)


def test_extract_chain_and_runs(lz):
    n = 20000
    F, T = chain_stream(n)
    assert np.array_equal(lz.decode(F, n), T)
    for pos, ln in ((n - 100, 100), (0, n), (4095, 2), (n - 1, 1)):
        assert np.array_equal(lz.extract(F, n, pos, ln), T[pos:pos + ln])
    for n in (4, 4097, 3 * 4096 + 5):
        for F, T in (run_stream(n), period3_stream(n)):
            for pos, ln in ranges(n, n):
                assert np.array_equal(lz.extract(F, n, pos, ln), T[pos:pos + ln]), (n, pos, ln)


def test_extract_rejects_invalid(lz):
    for F, n in invalid_streams():
        with pytest.raises(lz.Lz77SssError) as e:
            lz.extract(F, n, 0, n)
        assert e.value.code == lz.EINVAL
    F, T = run_stream(100)
    for pos, ln in ((0, 101), (100, 1), (101, 0), (1 << 63, 1 << 63), ((1 << 64) - 1, 2)):
        with pytest.raises(lz.Lz77SssError) as e:
            lz.extract(F, 100, pos, ln)
        assert e.value.code == lz.EINVAL
    assert lz.extract(np.zeros((0, 2), np.uint32), 0, 0, 0).size == 0
    assert lz.extract(F, 100, 100, 0).size == 0


def test_device_forms_check_arguments_first(lz):
    """pos + len > n is EINVAL whether or not a device is present (ENODEV only for a valid call)."""
    F, T = run_stream(100)
    for Fx in (F, F.astype(np.uint64)):
        for pos, ln in ((0, 101), (100, 1), ((1 << 64) - 1, 2)):
            with pytest.raises(lz.Lz77SssError) as e:
                lz.extract_device(Fx, 100, pos, ln)
            assert e.value.code == lz.EINVAL
        with pytest.raises(lz.Lz77SssError) as e:  # factors for an empty text
            lz.decode_device_windowed(Fx[:1], 0)
        assert e.value.code == lz.EINVAL
        assert lz.extract_device(Fx, 100, 50, 0).size == 0  # nothing to do: no device needed
        assert lz.decode_device_windowed(Fx[:0], 0).size == 0
    if lz.load_library().lz77sss_device_count() == 0:
        for call in (lambda: lz.extract_device(F, 100, 0, 100), lambda: lz.decode_device_windowed(F, 100)):
            with pytest.raises(lz.Lz77SssError) as e:
                call()
            assert e.value.code == lz.ENODEV


CPP_CLIENT = r"""
#include "lz77_sss.hpp"
#include <iterator>
#include <string>
#include <vector>
int main() {
    using L = lz77_sss<uint32_t>;
    std::vector<L::factor> F = {{'x', 0}, {'y', 0}, {'z', 0}, {0, 97}};
    std::string all, part;
    L::decode(F.begin(), std::back_inserter(all), 100);
    L::extract(F.begin(), std::back_inserter(part), 100, 31, 50);
    using W = lz77_sss<uint64_t>;
    std::vector<W::factor> G = {{'x', 0}, {'y', 0}, {'z', 0}, {0, 97}};
    std::string wide;
    W::extract(G.begin(), std::back_inserter(wide), 100, 31, 50);
    try {
        L::extract(F.begin(), std::back_inserter(part), 100, 60, 41);
        return 3;
    } catch (const lz77_sss_error& e) {
        if (e.code != LZ77SSS_EINVAL) return 4;
    }
    return part == all.substr(31, 50) && wide == part ? 0 : 1;
}
"""


def test_cpp_mirror_extract(lz, tmp_path):
    """lz77_sss<pos_t>::extract of the C++ mirror (host form: runs without a device)."""
    src = tmp_path / "extract_client.cpp"
    src.write_text(CPP_CLIENT)
    exe = tmp_path / "extract_client"
    libdir = ROOT / "lz77-sss_amd" / "lib"
    subprocess.run(["g++", "-O1", "-std=c++20", f"-I{ROOT / 'lz77-sss_amd' / 'host'}", str(src), "-o", str(exe),
                    f"-L{libdir}", "-llz77sss_hip", f"-Wl,-rpath,{libdir}"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
