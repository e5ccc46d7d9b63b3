// decode_win.hip -- LZ77 decode in bounded device memory: the windowed decode
// of a whole text, and the extraction of a byte range without decoding the text before it.
//
// decode_device (csrc/decode.hip) resolves all n positions at once and keeps 16 B (pos_t =
// uint32_t) or 24 B (uint64_t) per position.  Here the text is decoded left to right in windows
// of W positions: a copy whose folded source lies before the window reads a byte that is
// already final, so only the references that stay inside the window are pointer-jumped, over
// two u32 arrays of W entries.  Scratch is 8 B x W + 8 B x (nf + 1), whatever n is.
//
// Every stream is validated first, over its factors: the lengths sum to n (64-bit scan) and
// every copy has src < start.  After that every reference points strictly backwards, which is
// what makes the window order, the pointer jumping and the extract walk terminate.
#include "../../include/lz77sss.h"
#include "../include/engine.h"
#include "../include/prim.h"

namespace LZ_NS {

__global__ void k_dw_lens(const pos_t* __restrict__ F, u64 nf, u64* __restrict__ len) {
    for (u64 f = gtid(); f <= nf; f += gstride()) len[f] = f == nf ? 0 : (F[2 * f + 1] ? (u64)F[2 * f + 1] : 1u);
}
// per factor: it ends inside the text (so the 64-bit running sum never wrapped and the starts are
// strictly increasing) and a copy's source lies before its start
__global__ void k_dw_check(const pos_t* __restrict__ F, const u64* __restrict__ start, u64 nf, u64 n,
                           u32* __restrict__ err) {
    bool bad = false;
    for (u64 f = gtid(); f < nf; f += gstride()) {
        const u64 st = start[f];
        const u64 len = F[2 * f + 1] ? (u64)F[2 * f + 1] : 1u;
        bad |= st >= n || len > n - st || (F[2 * f + 1] != 0 && (u64)F[2 * f] >= st);
    }
    if (bad) atomicOr(err, 1u);  // only on an invalid stream
}

// the factor of position p (start st, source src, a copy): the position p's byte is copied from.
// A self-overlapping copy (distance d < len) is d-periodic: the offset is folded into the first
// period, so the source lies before the factor start
__device__ __forceinline__ u64 dw_source(u64 p, u64 st, u64 src) {
    const u64 d = st - src;
    u64 off = p - st;
    if (off >= d) off %= d;
    return src + off;
}

// Window [a, b) of the text, one workgroup per WB-position block (b - a <= 2^31, a a multiple of
// WB).  The factors covering a block are found as k_verify_blocks finds them: a binary search of
// the starts for the first one, the in-block starts marked in LDS, an inclusive max-scan; the
// scanned ids go back to LDS so that the positions are then visited lane by lane (coalesced).
// ref[p - a] = p - a for a terminal position (its byte is written here: a literal, or a copy from
// before the window, whose byte an earlier window made final), else the window-relative source.
constexpr u32 WB_T = 256, WB_PER = 16, WB = WB_T * WB_PER;
__global__ __launch_bounds__(WB_T) void k_dw_refs(const pos_t* __restrict__ F, const u64* __restrict__ start, u64 nf,
                                                   u64 a, u64 b, u8* out, u32* __restrict__ ref) {
    __shared__ u16 fl[WB];
    __shared__ u64 s_f0;
    __shared__ u32 s_wmax[WB_T / 64];
    const u64 nblk = (b - a + WB - 1) / WB;
    for (u64 blk = blockIdx.x; blk < nblk; blk += gridDim.x) {  // (block-uniform loop: barriers inside)
        const u64 b0 = a + blk * WB;
        const u64 b1 = min(b, b0 + WB);
        if (threadIdx.x == 0) {
            u64 lo = 0, hi = nf;  // last factor with start <= b0
            while (hi - lo > 1) {
                const u64 mid = (lo + hi) >> 1;
                if (start[mid] <= b0) lo = mid; else hi = mid;
            }
            s_f0 = lo;
        }
        for (u32 k = threadIdx.x; k < WB; k += WB_T) fl[k] = 0;
        __syncthreads();
        const u64 f0 = s_f0;
        // factors starting inside the block: at most WB of them, in order from f0 + 1
        for (u64 f = f0 + 1 + threadIdx.x; f < nf && start[f] < b1; f += WB_T) fl[start[f] - b0] = (u16)(f - f0);
        __syncthreads();
        const u32 base = threadIdx.x * WB_PER;
        u32 m = 0;
        for (u32 k = 0; k < WB_PER; k++) m = max(m, (u32)fl[base + k]);  // (fl[0] = 0: f0 covers b0)
        const u32 lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        u32 incl = m;
        for (u32 o = 1; o < 64; o <<= 1) {
            const u32 y = __shfl_up(incl, o, 64);
            if (lane >= o) incl = max(incl, y);
        }
        if (lane == 63) s_wmax[wv] = incl;
        __syncthreads();
        u32 carry = 0;
        for (u32 w = 0; w < wv; w++) carry = max(carry, s_wmax[w]);
        const u32 ex = (u32)__shfl_up(incl, 1, 64);
        u32 run = max(carry, lane ? ex : 0u);
        for (u32 k = 0; k < WB_PER; k++) {  // (a thread reads and writes only its own WB_PER entries)
            run = max(run, (u32)fl[base + k]);
            fl[base + k] = (u16)run;
        }
        __syncthreads();
        for (u32 k = 0; k < WB_PER; k++) {
            const u32 j = k * WB_T + threadIdx.x;
            const u64 p = b0 + j;
            if (p >= b1) break;
            const u64 f = f0 + fl[j];
            const pos_t src = F[2 * f], len = F[2 * f + 1];
            u32 r = (u32)(p - a);
            if (len == 0) {
                out[p] = (u8)src;
            } else {
                const u64 q = dw_source(p, start[f], (u64)src);
                if (q < a) out[p] = out[q];
                else r = (u32)(q - a);
            }
            ref[p - a] = r;
        }
        __syncthreads();  // fl / s_f0 / s_wmax are rewritten by the next block of the loop
    }
}

// one pointer-jumping round over the window's references (the shape of k_dec_jump: a fixed grid,
// one atomic per block for the change flag, four independent gathers in flight per lane)
constexpr unsigned DW_GRID = 4096;
__global__ void __launch_bounds__(256) k_dw_jump(const u32* __restrict__ ref, u32 w, u32* __restrict__ out,
                                                 u32* __restrict__ changed) {
    __shared__ u32 any;
    if (threadIdx.x == 0) any = 0;
    __syncthreads();
    bool ch = false;
    const u64 stride = (u64)gridDim.x * blockDim.x;
    u64 p = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; p + 3 * stride < w; p += 4 * stride) {
        u32 r[4], rr[4];
#pragma unroll
        for (int k = 0; k < 4; k++) r[k] = ref[p + k * stride];
#pragma unroll
        for (int k = 0; k < 4; k++) rr[k] = ref[r[k]];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            out[p + k * stride] = rr[k];
            ch |= rr[k] != r[k];
        }
    }
    for (; p < w; p += stride) {
        const u32 r = ref[p];
        const u32 rr = ref[r];
        out[p] = rr;
        ch |= rr != r;
    }
    if (ch) any = 1;
    __syncthreads();
    if (threadIdx.x == 0 && any) atomicOr(changed, 1u);
}
// the window's bytes: a non-terminal position copies its terminal's byte.  Only terminals are
// read and only non-terminals are written; with a compare text the differing positions are counted
__global__ void __launch_bounds__(256) k_dw_bytes(const u32* __restrict__ ref, u32 w, const u8* __restrict__ cmp,
                                                  u8* win /* out + a */, unsigned long long* __restrict__ mism) {
    u64 bad = 0;
    for (u64 i = gtid(); i < w; i += gstride()) {
        const u32 r = ref[i];
        const u8 c = win[r];
        if (r != (u32)i) win[i] = c;
        if (cmp) bad += cmp[i] != c;
    }
    if (cmp) {  // (wave-uniform)
        for (int o = 32; o > 0; o >>= 1) bad += __shfl_down(bad, o, 64);
        if ((threadIdx.x & 63) == 0 && bad) atomicAdd(mism, (unsigned long long)bad);  // only on a failed round trip
    }
}

// Range extract: lane i walks the reference chain of position pos + i down to a literal.  Every
// hop finds the factor covering the position.  Neighbouring lanes hold neighbouring positions and
// stay inside one factor until a factor boundary splits them, so per hop the factor of the lowest
// active lane is searched once for the wave and every lane tests its position against it; only
// the lanes that fail search themselves, on the side of that factor their position lies.  A lane
// that would pass max_hops hops stops and raises flags[0]; flags[1] = the largest hop count.
//
// The searches are shortened by a position index of the starts: idx[b] = the factor covering
// position b * WB (b <= nblk; idx[nblk] = nf - 1), so the factor of p lies in
// [idx[p / WB], idx[p / WB + 1]] -- as many search levels as log2 of the factors of one block, not log2 z.
__global__ void k_dw_index(const u64* __restrict__ start, u64 nf, u64 nblk, u64* __restrict__ idx) {
    for (u64 b = gtid(); b <= nblk; b += gstride()) {
        u64 lo = 0, hi = nf;  // last factor with start <= b * WB
        if (b == nblk) lo = nf - 1, hi = nf;
        while (hi - lo > 1) {
            const u64 mid = (lo + hi) >> 1;
            if (start[mid] <= b * WB) lo = mid; else hi = mid;
        }
        idx[b] = lo;
    }
}
__global__ __launch_bounds__(256) void k_dw_walk(const pos_t* __restrict__ F, const u64* __restrict__ start,
                                                  const u64* __restrict__ idx, u64 pos, u64 len, u32 max_hops,
                                                  u8* __restrict__ out, u32* __restrict__ flags) {
    u32 hmax = 0;
    bool ovf = false;
    const u64 span = (u64)gridDim.x * blockDim.x;
    for (u64 i0 = (u64)blockIdx.x * blockDim.x; i0 < len; i0 += span) {  // (block-uniform)
        const u64 i = i0 + threadIdx.x;
        bool active = i < len;
        u64 p = pos + i;
        u32 hops = 0;
        for (;;) {
            const u64 am = __ballot(active);
            if (!am) break;
            const u64 pl = __shfl(p, __ffsll((unsigned long long)am) - 1, 64);
            u64 lo = idx[pl / WB], hi = idx[pl / WB + 1] + 1;  // last factor with start <= pl (the same search in every lane)
            while (hi - lo > 1) {
                const u64 mid = (lo + hi) >> 1;
                if (start[mid] <= pl) lo = mid; else hi = mid;
            }
            if (active) {
                u64 f = lo, st = start[f];
                const u64 en = start[f + 1];
                if (p < st || p >= en) {
                    if (p < st) { lo = idx[p / WB]; hi = min(f, idx[p / WB + 1] + 1); }
                    else { lo = max(f + 1, idx[p / WB]); hi = idx[p / WB + 1] + 1; }
                    while (hi - lo > 1) {
                        const u64 mid = (lo + hi) >> 1;
                        if (start[mid] <= p) lo = mid; else hi = mid;
                    }
                    f = lo;
                    st = start[f];
                }
                const pos_t src = F[2 * f], ln = F[2 * f + 1];
                if (ln == 0) {
                    out[i] = (u8)src;
                    active = false;
                } else if (hops >= max_hops) {
                    ovf = true;
                    active = false;
                } else {
                    hops++;
                    p = dw_source(p, st, (u64)src);
                }
            }
        }
        hmax = max(hmax, hops);
    }
    for (int o = 32; o > 0; o >>= 1) hmax = max(hmax, (u32)__shfl_down(hmax, o, 64));
    const bool any_ovf = __ballot(ovf) != 0;
    if ((threadIdx.x & 63) == 0) {
        if (hmax) atomicMax(flags + 1, hmax);
        if (any_ovf) atomicOr(flags, 1u);
    }
}
__global__ void k_dw_diff(const u8* __restrict__ x, const u8* __restrict__ y, u64 len, unsigned long long* __restrict__ mism) {
    u64 bad = 0;
    for (u64 i = gtid(); i < len; i += gstride()) bad += x[i] != y[i];
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_down(bad, o, 64);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(mism, (unsigned long long)bad);
}

// the starts of the nf factors (start[nf] = n) in dec_start64, after the checks that need no
// device (argument errors) and then the validation of the stream
const u64* engine::dw_starts(const pos_t* F, u64 nf, u64 n_out) {
    if (nf == 0 || nf > n_out) throw error(LZ77SSS_EINVAL, "factor count does not fit the text length");
    if (n_out > POS_MAX_N) throw error(LZ77SSS_EINVAL, "n too large for pos_t");
    u64* start = dec_start64.get(nf + 1);
    k_dw_lens<<<capped_grid(nf + 1, 256), 256, 0, st>>>(F, nf, start);
    excl_sum64(start, start, (u64)0, nf + 1, scan_tmp, st);  // (in place: 8 B per factor)
    u32* flags = counters.get(16);
    LZ_HIP(hipMemsetAsync(flags, 0, 16, st));
    k_dw_check<<<capped_grid(nf, 256), 256, 0, st>>>(F, start, nf, n_out, flags);
    LZ_HIP(hipGetLastError());
    u64 total = 0;
    u32 err = 0;
    hread rb(st);
    rb.add(&total, (const u64*)start + nf);
    rb.add(&err, (const u32*)flags);
    rb.sync();
    if (total != n_out) throw error(LZ77SSS_EINVAL, "factor lengths do not sum to n");
    if (err) throw error(LZ77SSS_EINVAL, "factor source not before its position");
    return start;
}

// W for a request of `window` positions (0: the library's choice) when n_dec positions are decoded
u64 engine::dw_window(u64 window, u64 n_dec) const {
    constexpr u64 W_MAX = 1ull << 31;
    const u64 need = std::min<u64>(W_MAX, (n_dec + WB - 1) / WB * WB);  // one window holds everything
    u64 W;
    if (window) {
        W = std::min<u64>(W_MAX, (std::min<u64>(window, W_MAX) + WB - 1) / WB * WB);
    } else {
        // the measured default, at most what a quarter of the free HBM holds at 8 B per
        // position (the buffers the session already has for it count as free)
        W = DW_DEFAULT_WINDOW;
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess) {
            const u64 room = ((u64)fr + (dw_ref.cap + dw_ref2.cap) * 4) / 4 / 8 / WB * WB;
            W = std::min(W, std::max<u64>(room, WB));
        }
    }
    return std::min(W, need);
}

// windows of W positions over [0, n_dec) of the text the (validated) stream encodes
u64 engine::dw_run(const pos_t* F, u64 nf, const u64* start, u64 n_dec, u64 W, u8* out, const u8* cmp) {
    u32* ref = dw_ref.get(W);
    u32* ref2 = dw_ref2.get(W);
    u32* flags = counters.get(16);
    unsigned long long* mism = (unsigned long long*)counters64.get(24) + 16;  // (0..15: the greedy's slots)
    if (cmp) LZ_HIP(hipMemsetAsync(mism, 0, 8, st));
    dec_rounds = 0;
    dw_windows = 0;
    for (u64 a = 0; a < n_dec; a += W) {
        const u64 b = std::min(n_dec, a + W);
        const u32 w = (u32)(b - a);
        k_dw_refs<<<capped_grid(w, WB), WB_T, 0, st>>>(F, start, nf, a, b, out, ref);
        u32 rounds = 0;
        for (int round = 0; round < 40; round++) {  // (chains inside a window are shorter than 2^31)
            rounds++;
            LZ_HIP(hipMemsetAsync(flags + 1, 0, 4, st));
            k_dw_jump<<<std::min<u64>(cdiv(w, 256), DW_GRID), 256, 0, st>>>(ref, w, ref2, flags + 1);
            std::swap(ref, ref2);
            if (!rd1(flags + 1, st)) break;
        }
        dec_rounds = std::max(dec_rounds, rounds);
        dw_windows++;
        k_dw_bytes<<<std::min<u64>(cdiv(w, 256), 4 * DW_GRID), 256, 0, st>>>(ref, w, cmp ? cmp + a : nullptr, out + a, mism);
        LZ_HIP(hipGetLastError());
    }
    return cmp ? rd1((const u64*)mism, st) : 0;
}

// decodes nf factors (device array) of a text of length n_out into out (device, n_out bytes) in
// windows of `window` positions; with cmp, returns the number of positions that differ from it.
// Throws on an invalid stream before any byte is written.
u64 engine::decode_windowed(const pos_t* F, u64 nf, u64 n_out, u64 window, u8* out, const u8* cmp) {
    if (n_out == 0) {
        if (nf) throw error(LZ77SSS_EINVAL, "factors for an empty text");
        return 0;
    }
    const u64* start = dw_starts(F, nf, n_out);
    return dw_run(F, nf, start, n_out, dw_window(window, n_out), out, cmp);
}

// bytes [pos, pos + len) of the text the stream encodes, without the text before them: the walk
// kernel (over a position index of the starts, 8 B per 4096 bytes of [0, pos + len)), or -- when a
// chain passes the hop budget (LZ77SSS_EXTRACT_MAX_HOPS, read per call) or the range is long and
// most of its prefix -- the windowed decode of [0, pos + len), correct for every valid stream.  Returns the device
// bytes; info[0] = the path (LZ77SSS_EXTRACT_*), info[1] = the largest hop count of the walk.
const u8* engine::extract_device(const pos_t* F, u64 nf, u64 n_tot, u64 pos, u64 len, const u8* cmp, u64* mism,
                                 u64* info) {
    if (pos > n_tot || len > n_tot - pos) throw error(LZ77SSS_EINVAL, "range past the end of the text");
    if (n_tot == 0 && nf) throw error(LZ77SSS_EINVAL, "factors for an empty text");
    info[0] = LZ77SSS_EXTRACT_NONE;
    info[1] = 0;
    if (mism) *mism = 0;
    if (len == 0) return nullptr;
    u64 budget = DW_DEFAULT_MAX_HOPS;
    if (const char* e = std::getenv("LZ77SSS_EXTRACT_MAX_HOPS")) budget = std::strtoull(e, nullptr, 10);
    const u64* start = dw_starts(F, nf, n_tot);
    u32* flags = counters.get(16);  // (dw_starts zeroed them)
    // a long range that is a large part of its prefix is cheaper decoded than walked (the measured
    // crossover): no walk then
    const bool direct = len >= DW_DIRECT_MIN_LEN && pos + len <= DW_DIRECT_RATIO * len;
    u8* out = nullptr;
    u32 ovf = 0;
    if (!direct) {
        out = dw_ext.get(len);
        const u64 nblk = (pos + len + WB - 1) / WB;  // the walk stays below pos + len
        u64* idx = dw_idx.get(nblk + 1);
        k_dw_index<<<capped_grid(nblk + 1, 256), 256, 0, st>>>(start, nf, nblk, idx);
        k_dw_walk<<<(unsigned)std::min<u64>(cdiv(len, 256), 4 * DW_GRID), 256, 0, st>>>(
            F, start, idx, pos, len, (u32)std::min<u64>(budget, 0xFFFFFFFFu), out, flags);
        LZ_HIP(hipGetLastError());
        const auto [o, hmax] = rd2((const u32*)flags, (const u32*)flags + 1, st);
        ovf = o;
        info[0] = LZ77SSS_EXTRACT_WALK;
        info[1] = hmax;
    }
    if (direct || ovf) {
        const u64 n_dec = pos + len;
        u8* all = dec_out.get(n_dec);
        dw_run(F, nf, start, n_dec, dw_window(0, n_dec), all, nullptr);
        out = all + pos;
        info[0] = LZ77SSS_EXTRACT_PREFIX_DECODE;
    }
    if (cmp && mism) {
        unsigned long long* cnt = (unsigned long long*)counters64.get(24) + 16;
        LZ_HIP(hipMemsetAsync(cnt, 0, 8, st));
        k_dw_diff<<<capped_grid(len, 256), 256, 0, st>>>(out, cmp + pos, len, cnt);
        LZ_HIP(hipGetLastError());
        *mism = rd1((const u64*)cnt, st);
    }
    return out;
}

}  // namespace LZ_NS
