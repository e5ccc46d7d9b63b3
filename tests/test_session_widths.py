"""The C-ABI entry points whose answer depends on the session's position width (csrc/capi.hip reads
engine_if::pos_bytes): the widening accessors of a 32-bit session, the factor size of the
device-to-device copy, which sync set a 64-bit session's get_sss64 returns, and the number of
entries lz77sss_session_stats reports after each kind of call."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_P = ctypes.c_void_p


@pytest.fixture(scope="module")
def text(lz):
    return lz.gen_random_repetitive(20000, 20000, 1)


@pytest.fixture(scope="module")
def sess(lz, text):
    """(32-bit session, 64-bit session), the text loaded into both."""
    with lz.Session(1 << 16) as s32, lz.Session(1 << 16, pos64=True) as s64:
        s32.load(text)
        s64.load(text)
        yield s32, s64


def test_u32_session_widening_accessors(lz, sess):
    s, _ = sess
    lib = lz.load_library()
    z = s.factorize()
    F = s.factors(z)
    assert z > 0 and F.dtype == np.uint32
    F64 = np.empty((z, 2), np.uint64)
    assert lib.lz77sss_session_get_factors64(s._h, F64.ctypes.data_as(_P), z) == 0
    assert np.array_equal(F64, F.astype(np.uint64))
    L = s.lpf()
    assert L.shape[0] > 0 and L.dtype == np.uint32
    c = ctypes.c_uint64()
    L64 = np.empty((L.shape[0], 3), np.uint64)
    assert lib.lz77sss_session_get_lpf64(s._h, L64.ctypes.data_as(_P), L.shape[0], ctypes.byref(c)) == 0
    assert c.value == L.shape[0] and np.array_equal(L64, L.astype(np.uint64))
    assert s.factor_bytes() == 8 * z


def test_u64_session_factor_bytes(sess):
    _, s = sess
    z = s.factorize()
    assert z > 0 and s.factor_bytes() == 16 * z


def test_u64_get_sss64_follows_the_last_sync_set_call(sess):
    """get_sss64 of a 64-bit session: the text's own S after sss, the range's set after sss_range."""
    s32, s64 = sess
    full = s32.sss()[0].astype(np.uint64)
    first, end, base = 777, 15001, 1 << 40
    want = full[(full >= first) & (full < end)] + np.uint64(base)
    assert 0 < want.size < full.size
    c, _ = s64.sss_range(first, end, base=base)
    own, _ = s64.sss()
    assert np.array_equal(own, full)
    c, _ = s64.sss_range(first, end, base=base)
    assert c == want.size and np.array_equal(s64.sync_set64(c), want)
    s64.factorize()  # a factorization builds the text's own S again
    assert np.array_equal(s64.sync_set64(full.size), full)


@pytest.mark.parametrize("pos64", [False, True])
def test_stats_entry_counts(lz, text, pos64):
    """Entries of lz77sss_session_stats after each kind of call, as measured on the build before the
    C-ABI moved to csrc/capi.hip (both widths alike)."""
    with lz.Session(1 << 16, pos64=pos64) as s:
        assert len(s.stats()) == 0
        s.load(text)
        s.factorize()
        assert len(s.stats()) == 28
        s.decode()
        assert len(s.stats()) == 28
        s.extract(100, 1000)
        assert len(s.stats()) == 31
