"""The emitter's work counters (stats()[12:24], csrc/greedy.hip) on the C1 shape, per setting and
position width.  The factor streams are pinned elsewhere; these pin how the emitter got there:
outer rounds, walk rounds, segments walked, segment counts, sequential completion, windows, redos.
A change that walks segments twice or takes the sequential path where it did not keeps every
stream equal and shows only here.

The constants were recorded on the build before factorize_greedy was split into per-window steps
(each case run twice on each width; every entry repeated).  Entries: 12 outer rounds, 13 walk
rounds, 14 SSS fallback lanes, 15 segments walked, 16 final segment count, 17 default segments,
18 decode rounds, 19/20 sequential completion ran / from where, 21 windows, 22 SSS filter tiles,
23 windows walked again as the last."""
from __future__ import annotations

import pytest

pytestmark = pytest.mark.gpu

# setting -> (environment, stats[12:24] of the 32-bit session, of the 64-bit session)
CASES = {
    "default": ({},
                [3, 5, 0, 425, 203, 195, 0, 0, 0, 1, 13, 0],
                [3, 5, 0, 427, 203, 195, 0, 0, 0, 1, 13, 0]),
    "window": ({"LZ77SSS_GREEDY_WINDOW": "65536"},
               [8, 12, 0, 488, 64, 196, 0, 0, 0, 3, 13, 0],
               [8, 12, 0, 490, 64, 196, 0, 0, 0, 3, 13, 0]),
    "max_outer0": ({"LZ77SSS_GREEDY_MAX_OUTER": "0"},
                   [0, 0, 0, 0, 195, 195, 0, 1, 0, 1, 13, 0],
                   [0, 0, 0, 0, 195, 195, 0, 1, 0, 1, 13, 0]),
    "max_outer1": ({"LZ77SSS_GREEDY_MAX_OUTER": "1"},
                   [1, 2, 0, 202, 202, 195, 0, 1, 26909, 1, 13, 0],
                   [1, 2, 0, 202, 202, 195, 0, 1, 26909, 1, 13, 0]),
    "gap_chunk": ({"LZ77SSS_GAP_CHUNK": "64"},
                  [3, 6, 0, 1301, 686, 500, 0, 0, 0, 1, 13, 0],
                  [3, 6, 0, 1304, 686, 500, 0, 0, 0, 1, 13, 0]),
    "pred": ({"LZ77SSS_PRED": "1"},
             [3, 5, 0, 425, 203, 195, 0, 0, 0, 1, 13, 0],
             [3, 5, 0, 427, 203, 195, 0, 0, 0, 1, 13, 0]),
    "no_pred": ({"LZ77SSS_NO_PRED": "1"},
                [3, 5, 0, 425, 203, 195, 0, 0, 0, 1, 13, 0],
                [3, 5, 0, 427, 203, 195, 0, 0, 0, 1, 13, 0]),
}
Z = 735  # factors of the text (every setting gives the same stream)


@pytest.fixture(scope="module")
def sessions(lz):
    """(32-bit session, 64-bit session) with the C1 text of test_c1_seeds_vs_oracle (seed 1) loaded."""
    T = lz.gen_random_repetitive(10000, 200000, 1)
    with lz.Session(1 << 18) as s32, lz.Session(1 << 18, pos64=True) as s64:
        s32.load(T)
        s64.load(T)
        yield s32, s64


@pytest.mark.parametrize("pos64", [False, True], ids=["u32", "u64"])
@pytest.mark.parametrize("case", list(CASES))
def test_greedy_work_counters(sessions, monkeypatch, case, pos64):
    env, want32, want64 = CASES[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s = sessions[1 if pos64 else 0]
    z = s.factorize()
    got = [int(x) for x in s.stats()[12:24]]
    print(f"{case} pos64={pos64}: z={z} stats[12:24]={got}")
    assert z == Z
    assert got == (want64 if pos64 else want32)
