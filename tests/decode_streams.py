"""Factor streams shared by the windowed-decode and extract tests (test_decode_windowed.py on the
GPU, test_extract_host.py on the CPU): hand-built streams whose decoded text is known."""
from __future__ import annotations

import numpy as np


def run_stream(n):
    """'a' then one self-overlapping copy of distance 1 (n >= 2): text 'a' * n."""
    return np.array([[ord("a"), 0], [0, n - 1]], np.uint32), np.full(n, ord("a"), np.uint8)


def period3_stream(n):
    """Literals x y z then one copy of distance 3 (n >= 4)."""
    F = np.array([[120, 0], [121, 0], [122, 0], [0, n - 3]], np.uint32)
    return F, np.resize(np.array([120, 121, 122], np.uint8), n)


def chain_stream(n):
    """'a' then n - 1 copies (p - 1, 1): position p's chain has p hops, none of them foldable."""
    F = np.empty((n, 2), np.uint32)
    F[0] = (ord("a"), 0)
    F[1:, 0] = np.arange(n - 1, dtype=np.uint32)
    F[1:, 1] = 1
    return F, np.full(n, ord("a"), np.uint8)


def random_streams():
    """Arbitrary valid streams (not LZ77-greedy): random sources and lengths, the generator of
    test_device_decode_random_streams.  Yields (F, n)."""
    rng = np.random.default_rng(3)
    for n in [10, 1000, 100000]:
        F, pos = [], 0
        while pos < n:
            if pos == 0 or rng.random() < 0.3:
                F.append((int(rng.integers(0, 256)), 0)); pos += 1
            else:
                ln = int(min(n - pos, rng.integers(1, 2 * pos + 2)))
                F.append((int(rng.integers(0, pos)), ln)); pos += ln
        yield np.array(F, np.uint32), n


def invalid_streams():
    """(F, n) of test_device_decode_rejects_invalid: a forward reference, lengths that do not sum
    to n, factors for an empty text, lengths that sum to n + 2^32."""
    return [
        (np.array([[97, 0], [1, 2]], np.uint32), 3),
        (np.array([[97, 0], [0, 2]], np.uint32), 5),
        (np.array([[97, 0]], np.uint32), 0),
        (np.array([[97, 0], [0, 4], [0, 0xFFFFFFFF], [0, 1]], np.uint32), 5),
    ]


def factor_starts(F):
    """Start position of every factor, and the total length."""
    lens = np.maximum(np.asarray(F)[:, 1].astype(np.int64), 1)
    ends = np.cumsum(lens)
    return ends - lens, int(ends[-1]) if len(ends) else 0


def session_ranges(F, n, seed):
    """The (pos, len) ranges the session extract is checked on: the corners, a window boundary, a
    range inside the longest factor, one spanning at least three factors, 64 seeded random ones."""
    starts, total = factor_starts(F)
    assert total == n
    lens = np.maximum(F[:, 1].astype(np.int64), 1)
    R = [(0, 0), (0, 1), (n - 1, 1), (0, n), (4095, 2)]
    k = int(np.argmax(lens))
    R.append((int(starts[k]) + int(lens[k]) // 4, max(1, int(lens[k]) // 2)))
    m = len(F) // 2  # factors m - 1, m, m + 1
    assert 1 <= m <= len(F) - 2
    R.append((int(starts[m]) - 1, int(lens[m]) + 2))
    rng = np.random.default_rng(1000 + seed)
    for _ in range(64):
        p = int(rng.integers(0, n))
        R.append((p, int(rng.integers(0, min(n - p, 5000) + 1))))
    return R
