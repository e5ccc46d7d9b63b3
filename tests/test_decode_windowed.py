"""Windowed device decode and range extract (csrc/decode_win.hip) against the text itself, the
whole-text device decode and the host decode."""
from __future__ import annotations

import numpy as np
import pytest

from conftest import golden_names, load_golden
from decode_streams import (chain_stream, invalid_streams, period3_stream, random_streams, run_stream,
                            session_ranges)

pytestmark = pytest.mark.gpu

SEEDS = [1, 2, 3, 4]
_texts = {}


def rr_text(lz, seed):
    if seed not in _texts:
        _texts[seed] = lz.gen_random_repetitive(50000, 400000, seed)
    return _texts[seed]


def factorized(session, T):
    s = session(max(T.size, 1))
    s.load(T)
    z = s.factorize()
    return s, s.factors(z)


@pytest.mark.parametrize("name", golden_names())
def test_windowed_golden(lz, name):
    g = load_golden(name)
    T, F = g["text"], g["factors"]
    whole = lz.decode_device(F, T.size)
    for w in (4096, 8192, 0):
        D = lz.decode_device_windowed(F, T.size, w)
        assert np.array_equal(D, T), w
        assert np.array_equal(D, whole), w


@pytest.mark.parametrize("n", [4095, 4096, 4097, 3 * 4096 + 5, 1 << 20])
def test_windowed_self_overlap_across_windows(lz, n):
    for F, T in (run_stream(n), period3_stream(n)):
        D = lz.decode_device_windowed(F, n, 4096)
        assert np.array_equal(D, T)
        assert np.array_equal(lz.decode_device_windowed(F, n, 1), D)  # rounded up to 4096


def test_true_chain_depth(lz):
    """Every window's first position is external and the depth inside a window is 4096."""
    n = 20000
    F, T = chain_stream(n)
    assert np.array_equal(lz.decode_device_windowed(F, n, 4096), T)
    assert np.array_equal(lz.extract_device(F, n, n - 100, 100), T[n - 100:])
    assert np.array_equal(lz.extract_device(F, n, 0, n), T)


def test_windowed_random_streams(lz):
    for F, n in random_streams():
        T = lz.decode(F, n)
        assert np.array_equal(lz.decode_device_windowed(F, n, 4096), T)
        assert np.array_equal(lz.extract_device(F, n, n // 3, n - n // 3), T[n // 3:])


@pytest.mark.parametrize("seed", SEEDS)
def test_session_windowed_roundtrip(session, lz, seed):
    T = rr_text(lz, seed)
    s, _ = factorized(session, T)
    D, mism = s.decode_windowed(window=4096)
    assert mism == 0 and np.array_equal(D, T)
    D, mism = s.decode_windowed(out=False)
    assert D is None and mism == 0
    assert "decode" in s.phase_times()


def check_session_extract(lz, s, F, T, seed, path):
    for pos, ln in session_ranges(F, T.size, seed):
        assert np.array_equal(s.extract(pos, ln), T[pos:pos + ln]), (pos, ln)
        got = s.extract_info()[0]
        assert got == (lz.EXTRACT_NONE if ln == 0 else path(pos, ln)), (pos, ln, got)
    D, mism = s.extract(0, T.size, verify=True)
    assert mism == 0 and np.array_equal(D, T)
    assert "extract" in s.phase_times()
    with pytest.raises(lz.Lz77SssError) as e:
        s.extract(T.size - 1, 2)
    assert e.value.code == lz.EINVAL


@pytest.mark.parametrize("seed", SEEDS)
def test_session_extract(session, lz, seed):
    """With the default hop budget the greedy streams are answered by the walk."""
    T = rr_text(lz, seed)
    s, F = factorized(session, T)
    check_session_extract(lz, s, F, T, seed, lambda pos, ln: lz.EXTRACT_WALK)


def test_session64_windowed_and_extract(lz):
    T = rr_text(lz, 2)
    with lz.Session(T.size, pos64=True) as s:
        s.load(T)
        F = s.factors(s.factorize())
        assert F.dtype == np.uint64
        D, mism = s.decode_windowed(window=4096)
        assert mism == 0 and np.array_equal(D, T)
        check_session_extract(lz, s, F, T, 2, lambda pos, ln: lz.EXTRACT_WALK)
    assert np.array_equal(lz.decode_device_windowed(F, T.size, 8192), T)
    assert np.array_equal(lz.extract_device(F, T.size, 4095, 10000), T[4095:14095])


def chain_depths(F, n):
    """Hops of every position down to its literal (sources folded into the first period)."""
    depth = np.zeros(n, np.int64)
    p = 0
    for src, ln in F.astype(np.int64):
        if ln == 0:
            p += 1
            continue
        depth[p:p + ln] = np.resize(depth[src:src + min(p - src, ln)] + 1, ln)
        p += ln
    return depth


def test_extract_fallback_budget_1(session, lz, monkeypatch):
    """LZ77SSS_EXTRACT_MAX_HOPS=1: a range with a chain of two hops or more is answered by the windowed
    decode of the prefix, with the same bytes."""
    n = 20000
    Fc, Tc = chain_stream(n)
    monkeypatch.setenv("LZ77SSS_EXTRACT_MAX_HOPS", "1")
    for pos, ln in ((n - 100, 100), (0, n)):
        D, info = lz.extract_device(Fc, n, pos, ln, info=True)
        assert np.array_equal(D, Tc[pos:pos + ln]) and info == (lz.EXTRACT_PREFIX_DECODE, 1)
    D, info = lz.extract_device(Fc, n, 0, 2, info=True)  # a literal and one hop
    assert np.array_equal(D, Tc[:2]) and info == (lz.EXTRACT_WALK, 1)
    T = rr_text(lz, 1)
    s, F = factorized(session, T)
    depth = chain_depths(F, T.size)
    assert depth.max() >= 2
    deep = lambda pos, ln: lz.EXTRACT_PREFIX_DECODE if depth[pos:pos + ln].max() >= 2 else lz.EXTRACT_WALK
    assert deep(0, T.size) == lz.EXTRACT_PREFIX_DECODE
    check_session_extract(lz, s, F, T, 1, deep)
    monkeypatch.delenv("LZ77SSS_EXTRACT_MAX_HOPS")
    D, info = lz.extract_device(F, T.size, 0, T.size, info=True)
    assert np.array_equal(D, T) and info == (lz.EXTRACT_WALK, int(depth.max()))


def test_extract_long_range_decodes_prefix_directly(lz):
    """A range of 2^24 bytes or more that is at least half of its prefix is decoded, not walked
    (DESIGN.md 4.8); a range of the same length deeper in the text is walked."""
    ln = 1 << 24
    n = 2 * ln + 8
    F, T = period3_stream(n)
    for pos in (0, 5, ln):
        D, info = lz.extract_device(F, n, pos, ln, info=True)
        assert np.array_equal(D, T[pos:pos + ln]) and info == (lz.EXTRACT_PREFIX_DECODE, 0), pos
    D, info = lz.extract_device(F, n, ln + 1, ln, info=True)
    assert np.array_equal(D, T[ln + 1:2 * ln + 1]) and info == (lz.EXTRACT_WALK, 1)
    D, info = lz.extract_device(F, n, 0, ln - 1, info=True)
    assert np.array_equal(D, T[:ln - 1]) and info == (lz.EXTRACT_WALK, 1)


def test_rejects_invalid(lz):
    for F, n in invalid_streams():
        with pytest.raises(lz.Lz77SssError) as e:
            lz.decode_device_windowed(F, n, 4096)
        assert e.value.code == lz.EINVAL
        with pytest.raises(lz.Lz77SssError) as e:
            lz.extract_device(F, n, 0, n)
        assert e.value.code == lz.EINVAL
    F, T = run_stream(100)
    for pos, ln in ((0, 101), (100, 1), (101, 0), (1 << 63, 1 << 63), ((1 << 64) - 1, 2)):
        with pytest.raises(lz.Lz77SssError) as e:
            lz.extract_device(F, 100, pos, ln)
        assert e.value.code == lz.EINVAL
    empty = np.zeros((0, 2), np.uint32)
    assert lz.decode_device_windowed(empty, 0).size == 0
    assert lz.extract_device(empty, 0, 0, 0).size == 0
    assert lz.extract_device(F, 100, 100, 0).size == 0
    # a session without a factorization, or with a skip_phrases stream, has nothing to decode
    with lz.Session(1 << 16) as s:
        s.load(T)
        for call in (lambda: s.decode_windowed(), lambda: s.extract(0, 1)):
            with pytest.raises(lz.Lz77SssError) as e:
                call()
            assert e.value.code == lz.EINVAL
        s.factorize(fact_mode=lz.SKIP_PHRASES)
        for call in (lambda: s.decode_windowed(), lambda: s.extract(0, 1)):
            with pytest.raises(lz.Lz77SssError) as e:
                call()
            assert e.value.code == lz.EINVAL
