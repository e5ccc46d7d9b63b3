#!/usr/bin/env python3
"""Measurements of the bounded-memory decode (csrc/decode_win.hip).

  decode_bench.py --workload rr|genome [--size-mib 1024] [--lib other.so]
      The text of bench.py, factorized once on a pos_t = uint32_t session.  Times the whole-text
      decode (phase "decode" of Session.decode), the windowed decode at W in {2^20 .. 2^28} and at
      the library's default, and extracts of 1 MiB and 64 MiB at 16 seeded offsets (phase
      "extract", path, largest hop count).  One JSON line, also written to
      profiles/decode_windowed_<workload>.json.  --lib times only the whole-text decode with
      another build of the library (the parent commit's, for the A/B).
  decode_bench.py --big-gib 17
      A chr19-style text generated in HBM on a pos_t = uint64_t session, factorized, then
      decode_windowed(out=False, verify=True): mismatches, time and the peak device memory of the
      phase, appended to profiles/decode_windowed_17gib.txt.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "lz77-sss_amd"))


def timed(sess, call, phase, reps):
    """reps calls; the phase's device time of each (ms) and the last call's result."""
    ms, res = [], None
    for _ in range(reps):
        res = call()
        ms.append(sess.phase_times()[phase])
    return {"ms_min": round(min(ms), 3), "ms_median": round(statistics.median(ms), 3), "ms_all": [round(x, 3) for x in ms]}, res


def run_text(args, lz):
    from bench import make_text

    n = args.size_mib << 20
    t0 = time.time()
    T = make_text(lz, args.workload, n, 0)
    print(f"text {args.workload} n={n} generated in {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
    out = {"workload": args.workload, "n": n, "lib": str(args.lib or "this tree")}
    with lz.Session(n) as s:
        s.load(T)
        z = s.factorize()
        out["factors"] = z
        s.decode(out=False)  # warm-up: code objects, buffers
        r, (_, mism) = timed(s, lambda: s.decode(out=False), "decode", args.reps)
        out["whole"] = dict(r, mismatches=mism, jump_rounds=s.stats()[18])
        print(json.dumps({"whole": out["whole"]}), file=sys.stderr, flush=True)
        if args.lib:
            return out
        out["windowed"] = {}
        for w in [1 << 20, 1 << 22, 1 << 24, 1 << 26, 1 << 28, 0]:
            s.decode_windowed(window=w, out=False)
            r, (_, mism) = timed(s, lambda: s.decode_windowed(window=w, out=False), "decode", args.reps)
            out["windowed"]["default" if w == 0 else f"2^{w.bit_length() - 1}"] = dict(
                r, mismatches=mism, max_jump_rounds=s.stats()[18], vs_whole=round(r["ms_min"] / out["whole"]["ms_min"], 3))
            print(json.dumps({"window": w, **out["windowed"]["default" if w == 0 else f"2^{w.bit_length() - 1}"]}),
                  file=sys.stderr, flush=True)
        out["extract"] = {}
        rng = np.random.default_rng(11)
        for ln in (1 << 20, 64 << 20):
            if ln > n:
                continue
            by_path, hops, bad, samples = {}, 0, 0, []
            s.extract(n - ln, ln)
            for pos in [int(x) for x in rng.integers(0, n - ln + 1, 16)]:
                _, m = s.extract(pos, ln, verify=True)
                path, h = s.extract_info()
                ms = s.phase_times()["extract"]
                by_path.setdefault(path, []).append(ms)
                samples.append([pos, path, round(ms, 3)])
                hops, bad = max(hops, h), bad + m
            out["extract"][f"{ln >> 20}MiB"] = {
                "ms_by_path": {str(p): {"count": len(v), "min": round(min(v), 3), "median": round(statistics.median(v), 3),
                                        "max": round(max(v), 3)} for p, v in by_path.items()},
                "max_hops": hops, "mismatches": bad, "samples_pos_path_ms": samples}
        # the whole text through the walk, 8 MiB at a time (shorter than the ranges that are decoded
        # directly) and without a hop budget: the largest hop count any position of the stream reaches
        os.environ["LZ77SSS_EXTRACT_MAX_HOPS"] = str(2**32 - 1)
        hops, bad, ms = 0, 0, 0.0
        for pos in range(0, n, 8 << 20):
            _, m = s.extract(pos, min(8 << 20, n - pos), verify=True)
            hops, bad, ms = max(hops, s.extract_info()[1]), bad + m, ms + s.phase_times()["extract"]
        del os.environ["LZ77SSS_EXTRACT_MAX_HOPS"]
        out["extract"]["whole_text_walk"] = {"ms": round(ms, 3), "max_hops": hops, "mismatches": bad}
        # crossover: the walk costs per extracted byte, the prefix decode per byte of [0, pos + len)
        big = max(out["extract"], key=lambda k: int(k[:-3]) if k.endswith("MiB") else 0)
        walk = out["extract"][big]["ms_by_path"][str(lz.EXTRACT_WALK)]["median"] / int(big[:-3])  # ms per MiB extracted
        pref = out["windowed"]["default"]["ms_min"] / (n >> 20)                                     # ms per MiB decoded
        out["crossover"] = {"walk_ms_per_mib": round(walk, 5), "prefix_decode_ms_per_mib": round(pref, 5),
                            "prefix_cheaper_when_len_over_pos_plus_len_exceeds": round(pref / walk, 4)}
    return out


def run_big(args, lz):
    n = int(args.big_gib * (1 << 30))
    lines = [f"chr19-style text generated in HBM, n = {n} ({args.big_gib} GiB), pos_t = uint64_t session"]
    with lz.Session(n, pos64=True) as s:
        s.gen_genome(n, 59 << 20, 0.001, 7)
        t0 = time.time()
        z = s.factorize()
        lines.append(f"factorize: z = {z} in {time.time() - t0:.1f} s; verify (no decode) = {s.verify()} bad positions")
        t0 = time.time()
        _, mism = s.decode_windowed(out=False, verify=True)
        wall = time.time() - t0
        ms = s.phase_times()["decode"]
        mem = s.phase_mem()["decode"]
        lines.append(f"decode_windowed(window=0, out=False, verify=True): mismatches = {mism}, {ms:.1f} ms on the device "
                     f"({wall:.2f} s wall), max jump rounds per window = {s.stats()[18]}")
        lines.append(f"phase_mem decode: held = {mem['held'] / 2**30:.3f} GiB, peak = {mem['peak'] / 2**30:.3f} GiB, "
                     f"hbm_free = {mem['hbm_free'] / 2**30:.3f} GiB (held / peak: every engine buffer but the text, the "
                     f"n-byte output included; whole-text decode would add 24 B x n = {24 * n / 2**30:.0f} GiB)")
        _, m = s.extract(n - (64 << 20), 64 << 20, verify=True)
        lines.append(f"extract(n - 64 MiB, 64 MiB): mismatches = {m}, {s.phase_times()['extract']:.1f} ms, "
                     f"(path, max hops) = {s.extract_info()}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="rr", choices=["rr", "genome"])
    ap.add_argument("--size-mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lib", default=None, help="another build of liblz77sss_hip.so: whole-text decode only")
    ap.add_argument("--big-gib", type=float, default=0.0)
    ap.add_argument("--out-dir", default=str(ROOT / "profiles"))
    args = ap.parse_args()
    import lz77sss as lz

    if args.lib:  # (an older build lacks the newer entry points: bind what it has)
        have = ctypes.CDLL(args.lib)
        lz._SYMBOLS = {k: v for k, v in lz._SYMBOLS.items() if hasattr(have, k)}
        lz._lib = lz.load_library(args.lib)
    if lz.load_library().lz77sss_device_count() < 1:
        raise SystemExit("decode_bench: no GPU (there is no CPU fallback; nothing is measured)")
    outdir = Path(args.out_dir)
    outdir.mkdir(parents=True, exist_ok=True)
    if args.big_gib:
        lines = run_big(args, lz)
        print("\n".join(lines))
        with open(outdir / "decode_windowed_17gib.txt", "a") as f:
            f.write("\n".join(lines) + "\n")
        return
    out = run_text(args, lz)
    line = json.dumps(out)
    print(line)
    if not args.lib:
        (outdir / f"decode_windowed_{args.workload}.json").write_text(line + "\n")


if __name__ == "__main__":
    main()
