// capi.hip -- the device side of the C-ABI (include/lz77sss.h), compiled once.  A session owns
// one engine of either position width behind engine_if (include/engine_if.h); every entry point
// has one body written against that interface.  The host-only entry points (decode, extract,
// last_error) are csrc/host_codec.cpp.
#include "../../include/lz77sss.h"
#include "../include/engine.h"
#include "../include/engine_if.h"

#include <algorithm>
#include <memory>
#include <string>

struct lz77sss_session {
    std::unique_ptr<lz::engine_if> E;
    bool range64 = false;  // the last sync set came from sss_range (not sss / factorize)
};

namespace lz {
void set_last_error(const char* msg);  // csrc/host_codec.cpp
}

template <class F>
static int guarded(F&& f) {
    try {
        f();
        return LZ77SSS_OK;
    } catch (const lz::error& e) {
        lz::set_last_error(e.what());
        return e.code;
    } catch (const std::bad_alloc&) {
        lz::set_last_error("out of memory");
        return LZ77SSS_ENOMEM;
    } catch (const std::exception& e) {
        lz::set_last_error(e.what());
        return LZ77SSS_EINTERNAL;
    }
}
static void need32(lz77sss_session* s, const char* what) {
    if (s->E->pos_bytes() == 8) lz::not_on_pos64(what);
}

static void check_params(const lz77sss_params* prm) {
    if (!prm) throw lz::error(LZ77SSS_EINVAL, "params is NULL");
    if (prm->tau != 512) throw lz::error(LZ77SSS_EINVAL, "only tau = 512 is supported");
    if (prm->fact_mode != LZ77SSS_GREEDY && prm->fact_mode != LZ77SSS_SKIP_PHRASES)
        throw lz::error(LZ77SSS_EINVAL, "supported fact_modes: greedy, skip_phrases");
    if (prm->phr_mode < LZ77SSS_LPF_NAIVE || prm->phr_mode > LZ77SSS_LPF_LNF_OPT)
        throw lz::error(LZ77SSS_EINVAL, "unsupported phr_mode");
    if (prm->index_log2_size < 0 || prm->index_log2_size > 30) throw lz::error(LZ77SSS_EINVAL, "bad index_log2_size");
}

// factorize_exact<greedy, lpf_opt, transf_mode, range_ds_t, tau> (lz77_sss.hpp:188-200)
static void check_exact_params(const lz77sss_params* prm, int transf_mode) {
    if (!prm) throw lz::error(LZ77SSS_EINVAL, "params is NULL");
    if (prm->tau != 512) throw lz::error(LZ77SSS_EINVAL, "only tau = 512 is supported");
    if (prm->fact_mode != LZ77SSS_GREEDY) throw lz::error(LZ77SSS_EINVAL, "exact mode requires fact_mode = greedy");
    if (prm->phr_mode != LZ77SSS_LPF_OPT && prm->phr_mode != LZ77SSS_LPF_LNF_OPT)
        throw lz::error(LZ77SSS_EINVAL, "unsupported phr_mode");
    if (transf_mode < LZ77SSS_TRANSF_NAIVE || transf_mode > LZ77SSS_TRANSF_FULL_SA)
        throw lz::error(LZ77SSS_EINVAL, "unsupported transf_mode");
}

static int create_session(bool wide, int device, uint64_t max_n, lz77sss_session** out) {
    if (!out) return LZ77SSS_EINVAL;
    *out = nullptr;
    lz77sss_session* s = new (std::nothrow) lz77sss_session();
    if (!s) return LZ77SSS_ENOMEM;
    int rc = guarded([&] { s->E = wide ? lz64::make_engine(device, max_n) : lz::make_engine(device, max_n); });
    if (rc) {
        delete s;
        return rc;
    }
    *out = s;
    return LZ77SSS_OK;
}

// 64-bit sync set: the text's own S after sss / factorize on a 64-bit session, else the last
// sss_range result
static void sss64_src(lz77sss_session* s, const uint64_t*& p, uint64_t& cnt) {
    lz::engine_if& E = *s->E;
    if (E.pos_bytes() == 8 && !s->range64) {
        p = (const uint64_t*)E.sss_ptr();
        cnt = E.sss_size();
    } else {
        p = E.range_ptr();
        cnt = E.range_size();
    }
}

// chr19-style text in HBM: byte p of the text is a function of (p, seed) only
__device__ __forceinline__ lz::u64 gen_mix(lz::u64 x) {  // splitmix64 finalizer
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__global__ void k_gen_genome(lz::u8* __restrict__ out, lz::u64 n, lz::u64 offset, lz::u64 base_len,
                             lz::u64 mut_thr, lz::u64 seed) {
    for (lz::u64 i0 = lz::gtid() * 16; i0 < n; i0 += lz::gstride() * 16) {
    lz::u32 w[4] = {0, 0, 0, 0};
    for (int k = 0; k < 16 && i0 + k < n; k++) {
        const lz::u64 p = offset + i0 + k;
        const lz::u64 q = p % base_len;
        lz::u32 c = (lz::u32)(gen_mix(q ^ (seed << 40)) >> 62);
        if (p >= base_len) {
            const lz::u64 h = gen_mix(p ^ (seed * 0xD6E8FEB86659FD93ull) ^ 0x5851F42D4C957F2Dull);
            if (h < mut_thr) c = (c + 1 + (lz::u32)((h >> 7) % 3)) & 3;
        }
        w[k >> 2] |= (lz::u32)"ACGT"[c] << (8 * (k & 3));
    }
    if (i0 + 16 <= n) {
        *(uint4*)(out + i0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        for (int k = 0; i0 + k < n; k++) out[i0 + k] = (lz::u8)(w[k >> 2] >> (8 * (k & 3)));
    }
    }
}

extern "C" {

LZ77SSS_API int lz77sss_device_count(void) {
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) return 0;
    return c;
}

LZ77SSS_API void lz77sss_default_params(lz77sss_params* prm) {
    if (!prm) return;
    std::memset(prm, 0, sizeof(*prm));
    prm->phr_mode = LZ77SSS_LPF_OPT;
    prm->fact_mode = LZ77SSS_GREEDY;
    prm->tau = 512;
    prm->rk_seed = 42;
    prm->index_log2_size = 0;
    prm->device = 0;
    prm->log = 0;
    prm->num_threads = 0;
}

LZ77SSS_API int lz77sss_session_create(int device, uint64_t max_n, lz77sss_session** out) {
    return create_session(false, device, max_n, out);
}

LZ77SSS_API int lz77sss_session_create64(int device, uint64_t max_n, lz77sss_session** out) {
    return create_session(true, device, max_n, out);
}

LZ77SSS_API int lz77sss_session_is64(const lz77sss_session* s) { return s && s->E->pos_bytes() == 8 ? 1 : 0; }

LZ77SSS_API int lz77sss_session_load(lz77sss_session* s, const uint8_t* text, uint64_t n) {
    if (!s || (!text && n)) return LZ77SSS_EINVAL;
    return guarded([&] { s->E->load(text, n); });
}

LZ77SSS_API int lz77sss_session_factorize(lz77sss_session* s, const lz77sss_params* prm, uint64_t* num_factors) {
    if (!s) return LZ77SSS_EINVAL;
    return guarded([&] {
        check_params(prm);
        s->range64 = false;
        const uint64_t z = s->E->factorize(prm->phr_mode, prm->rk_seed, prm->index_log2_size, prm->log != 0,
                                           prm->fact_mode);
        if (num_factors) *num_factors = z;
    });
}

LZ77SSS_API int lz77sss_session_factorize_exact(lz77sss_session* s, const lz77sss_params* prm, int transf_mode,
                                                uint64_t* num_factors) {
    if (!s) return LZ77SSS_EINVAL;
    return guarded([&] {
        need32(s, "session_factorize_exact");
        check_exact_params(prm, transf_mode);
        // the reference's transforms run the sample-index path (csrc/smpl.hip); FULL_SA the
        // full suffix array (csrc/exact.hip)
        const uint64_t z = transf_mode == LZ77SSS_TRANSF_FULL_SA
                               ? s->E->factorize_exact(prm->log != 0)
                               : s->E->factorize_exact_smpl(transf_mode, prm->phr_mode, prm->rk_seed,
                                                            prm->index_log2_size, prm->log != 0);
        if (num_factors) *num_factors = z;
    });
}

LZ77SSS_API int lz77sss_session_get_factors(lz77sss_session* s, lz77sss_factor32* out, uint64_t cap) {
    if (!s) return LZ77SSS_EINVAL;
    return guarded([&] {
        need32(s, "get_factors (32-bit layout)");
        const uint64_t z = s->E->num_fact();
        if (!out && z) throw lz::error(LZ77SSS_EINVAL, "out is NULL");
        if (cap < z) throw lz::error(LZ77SSS_EINVAL, "output capacity too small");
        if (z) LZ_HIP(hipMemcpy(out, s->E->factors(), z * sizeof(lz77sss_factor32), hipMemcpyDeviceToHost));
    });
}

// the 10-byte serialized pos_t = uint64_t factor of lz77_sss.hpp:149-173 is a storage
// format; in memory a factor is {uint64_t src, uint64_t len} (lz77_sss.hpp:129-147)
LZ77SSS_API int lz77sss_session_get_factors64(lz77sss_session* s, lz77sss_factor64* out, uint64_t cap) {
    if (!s) return LZ77SSS_EINVAL;
    return guarded([&] {
        const uint64_t z = s->E->num_fact();
        if (!out && z) throw lz::error(LZ77SSS_EINVAL, "out is NULL");
        if (cap < z) throw lz::error(LZ77SSS_EINVAL, "output capacity too small");
        if (!z) return;
        if (s->E->pos_bytes() == 8) {
            LZ_HIP(hipMemcpy(out, s->E->factors(), z * sizeof(lz77sss_factor64), hipMemcpyDeviceToHost));
        } else {
            std::vector<lz77sss_factor32> tmp(z);
            LZ_HIP(hipMemcpy(tmp.data(), s->E->factors(), z * sizeof(lz77sss_factor32), hipMemcpyDeviceToHost));
            for (uint64_t k = 0; k < z; k++) out[k] = lz77sss_factor64{tmp[k].src, tmp[k].len};
        }
    });
}

// decode on the device: the factors of the last factorize call (already in HBM)
LZ77SSS_API int lz77sss_session_decode(lz77sss_session* s, uint8_t* out, uint64_t cap, uint64_t* mismatches) {
    if (!s) return LZ77SSS_EINVAL;
    return guarded([&] {
        lz::engine_if& E = *s->E;
        LZ_HIP(hipSetDevice(E.device()));
        if (out && cap < E.n()) throw lz::error(LZ77SSS_EINVAL, "output capacity too small");
        lz::u8* d_out = out && E.n() ? E.dec_out(E.n()) : nullptr;
        E.timer().begin(E.stream());
        const uint64_t bad = E.decode(E.factors(), E.num_fact(), E.n(), d_out, mismatches != nullptr);
        E.timer().mark("decode");
        if (E.stats().size() > lz::STAT_DEC_ROUNDS) E.stats()[lz::STAT_DEC_ROUNDS] = E.dec_rounds();
        if (mismatches) *mismatches = bad;
        if (d_out) LZ_HIP(hipMemcpyAsync(out, d_out, E.n(), hipMemcpyDeviceToHost, E.stream()));
        LZ_HIP(hipStreamSynchronize(E.stream()));
    });
}

// the factors of the last factorization checked against the loaded text in HBM (csrc/decode.hip
// verify_factors): the decode round trip without materialising the decoded text
LZ77SSS_API int lz77sss_session_verify(lz77sss_session* s, uint64_t* bad_positions, uint64_t* first_bad) {
    if (!s || !bad_positions) return LZ77SSS_EINVAL;
    return guarded([&] {
        s->E->check_verifiable();
        LZ_HIP(hipSetDevice(s->E->device()));
        *bad_positions = s->E->verify(first_bad);
    });
}

// the decode in bounded memory (csrc/decode_win.hip): the factors of the last factorization
LZ77SSS_API int lz77sss_session_decode_windowed(lz77sss_session* s, uint64_t window, uint8_t* out, uint64_t cap,
                                                uint64_t* mismatches) {
    if (!s) return LZ77SSS_EINVAL;
    return guarded([&] {
        lz::engine_if& E = *s->E;
        E.check_verifiable();
        if (out && cap < E.n()) throw lz::error(LZ77SSS_EINVAL, "output capacity too small");
        LZ_HIP(hipSetDevice(E.device()));
        lz::u8* d_out = E.n() ? E.dec_out(E.n()) : nullptr;
        E.timer().begin(E.stream());
        const uint64_t bad = E.decode_windowed(E.factors(), E.num_fact(), E.n(), window, d_out, mismatches != nullptr);
        E.timer().mark("decode");
        if (E.stats().size() > lz::STAT_DEC_ROUNDS) E.stats()[lz::STAT_DEC_ROUNDS] = E.dec_rounds();
        if (mismatches) *mismatches = bad;
        if (out && d_out) LZ_HIP(hipMemcpyAsync(out, d_out, E.n(), hipMemcpyDeviceToHost, E.stream()));
        LZ_HIP(hipStreamSynchronize(E.stream()));
    });
}

// bytes [pos, pos + len) of the last factorization's text (csrc/decode_win.hip extract_device)
LZ77SSS_API int lz77sss_session_extract(lz77sss_session* s, uint64_t pos, uint64_t len, uint8_t* out,
                                        uint64_t* mismatches) {
    if (!s || (!out && len)) return LZ77SSS_EINVAL;
    return guarded([&] {
        lz::engine_if& E = *s->E;
        const uint64_t n = E.n();
        E.check_verifiable();
        if (pos > n || len > n - pos) throw lz::error(LZ77SSS_EINVAL, "range past the end of the text");
        LZ_HIP(hipSetDevice(E.device()));
        uint64_t info[2] = {0, 0};
        E.timer().begin(E.stream());
        const lz::u8* d = E.extract(E.factors(), E.num_fact(), n, pos, len, mismatches != nullptr, mismatches, info);
        E.timer().mark("extract");
        std::vector<uint64_t>& stats = E.stats();
        if (stats.size() < lz::STAT_EXTRACT + 2) stats.resize(lz::STAT_EXTRACT + 2, 0);
        stats[lz::STAT_EXTRACT] = info[0];
        stats[lz::STAT_EXTRACT + 1] = info[1];
        if (d && len) LZ_HIP(hipMemcpyAsync(out, d, len, hipMemcpyDeviceToHost, E.stream()));
        LZ_HIP(hipStreamSynchronize(E.stream()));
    });
}

LZ77SSS_API int lz77sss_session_sss(lz77sss_session* s, uint64_t* size_sss, int* has_runs) {
    if (!s) return LZ77SSS_EINVAL;
    return guarded([&] {
        uint64_t sz = 0;
        int hr = 0;
        s->E->sss(&sz, &hr);
        s->range64 = false;
        if (size_sss) *size_sss = sz;
        if (has_runs) *has_runs = hr;
    });
}

LZ77SSS_API int lz77sss_session_sss_range(lz77sss_session* s, uint64_t first, uint64_t end, uint64_t base,
                                          uint64_t window, uint64_t* size_sss, int* has_runs) {
    if (!s) return LZ77SSS_EINVAL;
    return guarded([&] {
        uint64_t cnt = 0;
        int hr = 0;
        s->E->sss_range(first, end, base, window, &cnt, &hr);
        s->range64 = true;
        if (size_sss) *size_sss = cnt;
        if (has_runs) *has_runs = hr;
    });
}

LZ77SSS_API int lz77sss_session_get_sss64(lz77sss_session* s, uint64_t* out, uint64_t cap) {
    if (!s) return LZ77SSS_EINVAL;
    return guarded([&] {
        const uint64_t* p;
        uint64_t cnt;
        sss64_src(s, p, cnt);
        if (!out && cnt) throw lz::error(LZ77SSS_EINVAL, "out is NULL");
        if (cap < cnt) throw lz::error(LZ77SSS_EINVAL, "output capacity too small");
        if (cnt) LZ_HIP(hipMemcpy(out, p, cnt * 8, hipMemcpyDeviceToHost));
    });
}

LZ77SSS_API int lz77sss_session_copy_sss64_device(lz77sss_session* s, void* dst, uint64_t cap) {
    if (!s) return LZ77SSS_EINVAL;
    return guarded([&] {
        const uint64_t* p;
        uint64_t cnt;
        sss64_src(s, p, cnt);
        if (!dst && cnt) throw lz::error(LZ77SSS_EINVAL, "dst is NULL");
        if (cap < cnt) throw lz::error(LZ77SSS_EINVAL, "output capacity too small");
        hipStream_t st = s->E->stream();
        LZ_HIP(hipSetDevice(s->E->device()));
        if (cnt) LZ_HIP(hipMemcpyAsync(dst, p, cnt * 8, hipMemcpyDeviceToDevice, st));
        LZ_HIP(hipStreamSynchronize(st));
    });
}

// device-to-device copy of the last factorization in the session's own layout
// ({u32 src, u32 len} or {u64 src, u64 len} per factor): the emission step of a
// sharded run gathers these bytes over RCCL without a host round trip
LZ77SSS_API int lz77sss_session_copy_factors_device(lz77sss_session* s, void* dst, uint64_t cap_bytes,
                                                    uint64_t* bytes) {
    if (!s) return LZ77SSS_EINVAL;
    return guarded([&] {
        const uint64_t nb = s->E->num_fact() * 2 * s->E->pos_bytes();
        if (bytes) *bytes = nb;
        if (!dst) {
            if (cap_bytes) throw lz::error(LZ77SSS_EINVAL, "dst is NULL");
            return;
        }
        if (cap_bytes < nb) throw lz::error(LZ77SSS_EINVAL, "output capacity too small");
        hipStream_t st = s->E->stream();
        LZ_HIP(hipSetDevice(s->E->device()));
        if (nb) LZ_HIP(hipMemcpyAsync(dst, s->E->factors(), nb, hipMemcpyDefault, st));
        LZ_HIP(hipStreamSynchronize(st));
    });
}

LZ77SSS_API int lz77sss_session_gen_genome(lz77sss_session* s, uint64_t n, uint64_t base_len, double mut_rate,
                                           uint32_t seed, uint64_t offset) {
    if (!s || base_len == 0 || !(mut_rate >= 0.0 && mut_rate <= 1.0)) return LZ77SSS_EINVAL;
    return guarded([&] {
        lz::engine_if& E = *s->E;
        lz::u8* text = E.text();
        hipStream_t st = E.stream();
        if (n > E.max_n()) throw lz::error(LZ77SSS_EINVAL, "text larger than the session capacity");
        LZ_HIP(hipSetDevice(E.device()));
        E.set_n(n);
        const lz::u64 thr = mut_rate >= 1.0 ? ~0ull : (lz::u64)(mut_rate * 18446744073709551616.0);
        if (n) k_gen_genome<<<lz::capped_grid((n + 15) / 16, 256), 256, 0, st>>>(text, n, offset, base_len, thr, seed);
        LZ_HIP(hipGetLastError());
        LZ_HIP(hipMemsetAsync(text + n, 0, lz::TEXT_PAD, st));
        LZ_HIP(hipStreamSynchronize(st));
    });
}

// Huffman factor container of the last greedy / exact factorization (csrc/huffman.hip)
LZ77SSS_API int lz77sss_session_huffman(lz77sss_session* s, uint8_t* out, uint64_t cap, uint64_t* size) {
    if (!s) return LZ77SSS_EINVAL;
    return guarded([&] {
        need32(s, "huffman");
        lz::engine_if& E = *s->E;
        if (E.last_fact_mode() == LZ77SSS_SKIP_PHRASES)
            throw lz::error(LZ77SSS_EINVAL, "the Huffman container holds a factorization, not a skip_phrases stream");
        LZ_HIP(hipSetDevice(E.device()));
        const uint64_t b = E.huffman_container();
        if (size) *size = b;
        if (out) {
            if (cap < b) throw lz::error(LZ77SSS_EINVAL, "output capacity too small");
            LZ_HIP(hipMemcpy(out, E.huffman_out(), b, hipMemcpyDeviceToHost));
        }
    });
}

// ssszip's gapped container of the last skip_phrases factorization (csrc/ssszip.hip)
LZ77SSS_API int lz77sss_session_ssszip_gapped(lz77sss_session* s, uint8_t* out, uint64_t cap, uint64_t* size) {
    if (!s) return LZ77SSS_EINVAL;
    return guarded([&] {
        need32(s, "ssszip_gapped");
        lz::engine_if& E = *s->E;
        if (E.last_fact_mode() != LZ77SSS_SKIP_PHRASES)
            throw lz::error(LZ77SSS_EINVAL, "ssszip_gapped needs a preceding factorize with fact_mode = skip_phrases");
        LZ_HIP(hipSetDevice(E.device()));
        const uint64_t b = E.ssszip_gapped();
        if (size) *size = b;
        if (out) {
            if (cap < b) throw lz::error(LZ77SSS_EINVAL, "output capacity too small");
            LZ_HIP(hipMemcpy(out, E.ssszip_out(), b, hipMemcpyDeviceToHost));
        }
    });
}

LZ77SSS_API int lz77sss_session_get_sss(lz77sss_session* s, uint32_t* out, uint64_t cap) {
    if (!s) return LZ77SSS_EINVAL;
    return guarded([&] {
        need32(s, "get_sss (32-bit positions)");
        const uint64_t cnt = s->E->sss_size();
        if (cap < cnt) throw lz::error(LZ77SSS_EINVAL, "output capacity too small");
        if (cnt) LZ_HIP(hipMemcpy(out, s->E->sss_ptr(), (size_t)cnt * 4, hipMemcpyDeviceToHost));
    });
}

LZ77SSS_API int lz77sss_session_get_sa_s(lz77sss_session* s, uint32_t* sa, uint32_t* lcp, uint64_t cap) {
    if (!s) return LZ77SSS_EINVAL;
    return guarded([&] {
        const uint64_t cnt = s->E->sss_size();
        if (cap < cnt) throw lz::error(LZ77SSS_EINVAL, "output capacity too small");
        if (!cnt) return;
        if (sa) LZ_HIP(hipMemcpy(sa, s->E->sa_ptr(), (size_t)cnt * 4, hipMemcpyDeviceToHost));
        if (lcp) LZ_HIP(hipMemcpy(lcp, s->E->lcp_ptr(), (size_t)cnt * 4, hipMemcpyDeviceToHost));
    });
}

LZ77SSS_API int lz77sss_session_get_lpf(lz77sss_session* s, uint32_t* out3, uint64_t cap, uint64_t* count) {
    if (!s) return LZ77SSS_EINVAL;
    return guarded([&] {
        need32(s, "get_lpf (32-bit positions)");
        const uint64_t m = s->E->num_phr();
        if (count) *count = m;
        if (!out3) return;
        if (cap < m) throw lz::error(LZ77SSS_EINVAL, "output capacity too small");
        if (m) LZ_HIP(hipMemcpy(out3, s->E->lpf_ptr(), (size_t)m * 12, hipMemcpyDeviceToHost));
    });
}

LZ77SSS_API int lz77sss_session_get_lpf64(lz77sss_session* s, uint64_t* out3, uint64_t cap, uint64_t* count) {
    if (!s) return LZ77SSS_EINVAL;
    return guarded([&] {
        const uint64_t m = s->E->num_phr();
        if (count) *count = m;
        if (!out3 || !m) return;
        if (cap < m) throw lz::error(LZ77SSS_EINVAL, "output capacity too small");
        if (s->E->pos_bytes() == 8) {
            LZ_HIP(hipMemcpy(out3, s->E->lpf_ptr(), (size_t)m * 24, hipMemcpyDeviceToHost));
        } else {
            std::vector<uint32_t> tmp(3 * m);
            LZ_HIP(hipMemcpy(tmp.data(), s->E->lpf_ptr(), (size_t)m * 12, hipMemcpyDeviceToHost));
            for (uint64_t k = 0; k < 3 * m; k++) out3[k] = tmp[k];
        }
    });
}

LZ77SSS_API int lz77sss_session_phase_times(lz77sss_session* s, double* ms, const char** names, int cap) {
    if (!s) return LZ77SSS_EINVAL;
    int k = 0;
    int rc = guarded([&] {
        static thread_local std::vector<std::string> keep;
        auto v = s->E->timer().read();
        keep.clear();
        for (auto& x : v) keep.push_back(x.first);
        for (auto& x : v) {
            if (k >= cap) break;
            if (ms) ms[k] = x.second;
            if (names) names[k] = keep[k].c_str();
            k++;
        }
    });
    return rc ? rc : k;
}

// device memory per phase, in the order of lz77sss_session_phase_times
LZ77SSS_API int lz77sss_session_phase_mem(lz77sss_session* s, uint64_t* held, uint64_t* peak, uint64_t* hbm_free,
                                          int cap) {
    if (!s) return LZ77SSS_EINVAL;
    const lz::phase_timer& t = s->E->timer();
    int k = 0;
    for (size_t i = 1; i < t.mem.size() && k < cap; i++, k++) {
        if (held) held[k] = t.mem[i].held;
        if (peak) peak[k] = t.mem[i].peak;
        if (hbm_free) hbm_free[k] = t.mem[i].hbm_free;
    }
    return k;
}

LZ77SSS_API int lz77sss_session_stats(lz77sss_session* s, uint64_t* out, int cap) {
    if (!s || !out) return LZ77SSS_EINVAL;
    const std::vector<uint64_t>& st = s->E->stats();
    int k = 0;
    for (; k < cap && k < (int)st.size(); k++) out[k] = st[k];
    return k;
}

LZ77SSS_API int lz77sss_session_sss_kernel_time(lz77sss_session* s, double* ms, uint64_t* bytes) {
    if (!s) return LZ77SSS_EINVAL;
    if (ms) *ms = s->E->sss_kernel_ms();
    if (bytes) *bytes = s->E->sss_kernel_bytes();
    return LZ77SSS_OK;
}

LZ77SSS_API void lz77sss_session_destroy(lz77sss_session* s) { delete s; }

// ---- sharded factorization: sync set by text block + all-gather, the
// phrases on every rank, the greedy chain block by block in rank order
LZ77SSS_API int lz77sss_session_set_sss(lz77sss_session* s, const uint64_t* S, uint64_t count, int has_runs) {
    if (!s || (!S && count)) return LZ77SSS_EINVAL;
    return guarded([&] { s->E->set_sss(S, count, has_runs != 0); });
}

LZ77SSS_API int lz77sss_session_prepare(lz77sss_session* s, const lz77sss_params* prm, int external_sss,
                                        uint64_t* carried_bytes) {
    if (!s) return LZ77SSS_EINVAL;
    return guarded([&] {
        check_params(prm);
        const uint64_t b = s->E->prepare(prm->phr_mode, external_sss != 0, prm->index_log2_size);
        if (carried_bytes) *carried_bytes = b;
    });
}

LZ77SSS_API int lz77sss_session_carried_copy(lz77sss_session* s, void* buf, uint64_t bytes, int to_session) {
    if (!s || (!buf && bytes)) return LZ77SSS_EINVAL;
    return guarded([&] {
        void* tab = s->E->carried_table();
        if (!tab) throw lz::error(LZ77SSS_EINVAL, "no carried table: call lz77sss_session_prepare first");
        if (bytes > s->E->carried_bytes()) throw lz::error(LZ77SSS_EINVAL, "carried table smaller than the copy");
        hipStream_t st = s->E->stream();
        LZ_HIP(hipSetDevice(s->E->device()));
        if (bytes) {
            if (to_session) LZ_HIP(hipMemcpyAsync(tab, buf, bytes, hipMemcpyDefault, st));
            else LZ_HIP(hipMemcpyAsync(buf, tab, bytes, hipMemcpyDefault, st));
        }
        LZ_HIP(hipStreamSynchronize(st));
    });
}

LZ77SSS_API int lz77sss_session_greedy_block(lz77sss_session* s, const lz77sss_params* prm, lz77sss_block* blk,
                                             uint64_t* num_factors) {
    if (!s || !blk) return LZ77SSS_EINVAL;
    return guarded([&] {
        check_params(prm);
        // reserved = 1: seed the table from the gap positions before start (a speculative lead-in)
        uint64_t st[8] = {blk->start, blk->idxpos, blk->zmask,
                          (uint64_t)(blk->carried != 0) | (blk->reserved == 1 && !blk->carried ? 2u : 0u), blk->end, 0,
                          0, 0};
        const uint64_t z = s->E->greedy_block(prm->rk_seed, prm->index_log2_size, st);
        blk->exit_start = st[5];
        blk->exit_idxpos = st[6];
        blk->exit_zmask = (uint32_t)st[7];
        if (num_factors) *num_factors = z;
    });
}

LZ77SSS_API int lz77sss_session_spec_begin(lz77sss_session* s, int part, uint64_t block_start) {
    if (!s || part < 0 || part >= LZ77SSS_SPEC_MAX_PARTS) return LZ77SSS_EINVAL;
    return guarded([&] { s->E->spec_begin(part, block_start); });
}

LZ77SSS_API int lz77sss_session_spec_resolve(lz77sss_session* s, const void* true_table, uint64_t bytes, int parts,
                                             int* accepted_parts) {
    if (!s || !true_table || !accepted_parts || parts < 0 || parts > LZ77SSS_SPEC_MAX_PARTS) return LZ77SSS_EINVAL;
    return guarded([&] { *accepted_parts = s->E->spec_resolve(true_table, bytes, parts); });
}

}  // extern "C"

// one-shot: upload, factorize, stream the factors to the callback in text order
template <class FACT, class EMIT>
static int one_shot(const uint8_t* text, uint64_t n, const lz77sss_params* prm, EMIT emit, void* user, bool exact,
                    int transf_mode) {
    constexpr bool wide = sizeof(FACT) == 16;
    if ((!text && n) || !emit) return LZ77SSS_EINVAL;
    lz77sss_session* s = nullptr;
    int rc = guarded([&] {
        if (exact) check_exact_params(prm, transf_mode);
        else check_params(prm);
    });
    if (rc) return rc;
    rc = create_session(wide && !exact, prm->device, n, &s);
    if (rc) return rc;
    rc = lz77sss_session_load(s, text, n);
    uint64_t z = 0;
    if (!rc) rc = exact ? lz77sss_session_factorize_exact(s, prm, transf_mode, &z) : lz77sss_session_factorize(s, prm, &z);
    if (!rc && z) {
        std::vector<FACT> buf;
        rc = guarded([&] { buf.resize(z); });
        if (!rc) {
            if constexpr (wide) rc = lz77sss_session_get_factors64(s, buf.data(), z);
            else rc = lz77sss_session_get_factors(s, buf.data(), z);
        }
        const uint64_t B = 1 << 16;
        for (uint64_t o = 0; !rc && o < z; o += B) {
            if (emit(buf.data() + o, std::min(B, z - o), user) != 0) {
                lz::set_last_error("emit callback aborted");
                rc = LZ77SSS_ECALLBACK;
            }
        }
    }
    lz77sss_session_destroy(s);
    return rc;
}

// decode on a device: upload, pointer-jumping decode (csrc/decode.hip), download
template <class FACT>
static int one_shot_decode(const FACT* f, uint64_t nf, uint8_t* out, uint64_t n, int device) {
    if ((!f && nf) || (!out && n)) return LZ77SSS_EINVAL;
    lz77sss_session* s = nullptr;
    int rc = create_session(sizeof(FACT) == 16, device, n, &s);
    if (rc) return rc;
    rc = guarded([&] {
        lz::engine_if& E = *s->E;
        void* F = E.factors_buf(nf);
        if (nf) LZ_HIP(hipMemcpyAsync(F, f, nf * sizeof(FACT), hipMemcpyHostToDevice, E.stream()));
        lz::u8* d_out = n ? E.dec_out(n) : nullptr;
        E.decode(F, nf, n, d_out, false);
        if (n) LZ_HIP(hipMemcpyAsync(out, d_out, n, hipMemcpyDeviceToHost, E.stream()));
        LZ_HIP(hipStreamSynchronize(E.stream()));
    });
    lz77sss_session_destroy(s);
    return rc;
}

// one-shot forms of the bounded-memory decode and the range extract (csrc/decode_win.hip): the
// factors go up, the bytes come down; the session holds no text.  Argument errors are reported
// before the device is touched.  extract: bytes [pos, pos + len); else the whole text in windows
template <class FACT>
static int one_shot_decode_win(const FACT* f, uint64_t nf, uint64_t n, uint64_t window, bool extract, uint64_t pos,
                               uint64_t len, uint8_t* out, int device, uint64_t* info) {
    const uint64_t nout = extract ? len : n;
    int rc = guarded([&] {
        if ((!f && nf) || (!out && nout)) throw lz::error(LZ77SSS_EINVAL, "NULL argument");
        if (extract && (pos > n || len > n - pos)) throw lz::error(LZ77SSS_EINVAL, "range past the end of the text");
        if (n == 0 && nf) throw lz::error(LZ77SSS_EINVAL, "factors for an empty text");
        if (n && (nf == 0 || nf > n)) throw lz::error(LZ77SSS_EINVAL, "factor count does not fit the text length");
    });
    if (info) info[0] = LZ77SSS_EXTRACT_NONE, info[1] = 0;
    if (rc || nout == 0) return rc;
    lz77sss_session* s = nullptr;
    rc = create_session(sizeof(FACT) == 16, device, 0, &s);
    if (rc) return rc;
    rc = guarded([&] {
        lz::engine_if& E = *s->E;
        hipStream_t st = E.stream();
        uint64_t inf[2] = {0, 0};
        const lz::u8* d = nullptr;
        void* F = E.factors_buf(nf);
        LZ_HIP(hipMemcpyAsync(F, f, nf * sizeof(FACT), hipMemcpyHostToDevice, st));
        if (extract) {
            d = E.extract(F, nf, n, pos, len, false, nullptr, inf);
        } else {
            lz::u8* d_out = E.dec_out(n);
            E.decode_windowed(F, nf, n, window, d_out, false);
            d = d_out;
        }
        if (info) info[0] = inf[0], info[1] = inf[1];
        LZ_HIP(hipMemcpyAsync(out, d, nout, hipMemcpyDeviceToHost, st));
        LZ_HIP(hipStreamSynchronize(st));
    });
    lz77sss_session_destroy(s);
    return rc;
}

extern "C" {
LZ77SSS_API int lz77sss_factorize_approx_u32(const uint8_t* text, uint64_t n, const lz77sss_params* prm,
                                             lz77sss_emit_fn emit, void* user) {
    return one_shot<lz77sss_factor32>(text, n, prm, emit, user, false, 0);
}
LZ77SSS_API int lz77sss_factorize_approx_u64(const uint8_t* text, uint64_t n, const lz77sss_params* prm,
                                             lz77sss_emit64_fn emit, void* user) {
    return one_shot<lz77sss_factor64>(text, n, prm, emit, user, false, 0);
}
LZ77SSS_API int lz77sss_factorize_exact_u32(const uint8_t* text, uint64_t n, const lz77sss_params* prm,
                                            int transf_mode, lz77sss_emit_fn emit, void* user) {
    return one_shot<lz77sss_factor32>(text, n, prm, emit, user, true, transf_mode);
}
LZ77SSS_API int lz77sss_factorize_exact_u64(const uint8_t* text, uint64_t n, const lz77sss_params* prm,
                                            int transf_mode, lz77sss_emit64_fn emit, void* user) {
    return one_shot<lz77sss_factor64>(text, n, prm, emit, user, true, transf_mode);
}
LZ77SSS_API int lz77sss_decode_u32_device(const lz77sss_factor32* f, uint64_t nf, uint8_t* out, uint64_t n,
                                          int device) {
    return one_shot_decode(f, nf, out, n, device);
}
LZ77SSS_API int lz77sss_decode_u64_device(const lz77sss_factor64* f, uint64_t nf, uint8_t* out, uint64_t n,
                                          int device) {
    return one_shot_decode(f, nf, out, n, device);
}
LZ77SSS_API int lz77sss_decode_u32_device_windowed(const lz77sss_factor32* f, uint64_t nf, uint8_t* out, uint64_t n,
                                                   uint64_t window, int device) {
    return one_shot_decode_win(f, nf, n, window, false, 0, 0, out, device, nullptr);
}
LZ77SSS_API int lz77sss_decode_u64_device_windowed(const lz77sss_factor64* f, uint64_t nf, uint8_t* out, uint64_t n,
                                                   uint64_t window, int device) {
    return one_shot_decode_win(f, nf, n, window, false, 0, 0, out, device, nullptr);
}
LZ77SSS_API int lz77sss_extract_u32_device(const lz77sss_factor32* f, uint64_t nf, uint64_t n, uint64_t pos,
                                           uint64_t len, uint8_t* out, int device, uint64_t* info) {
    return one_shot_decode_win(f, nf, n, 0, true, pos, len, out, device, info);
}
LZ77SSS_API int lz77sss_extract_u64_device(const lz77sss_factor64* f, uint64_t nf, uint64_t n, uint64_t pos,
                                           uint64_t len, uint8_t* out, int device, uint64_t* info) {
    return one_shot_decode_win(f, nf, n, 0, true, pos, len, out, device, info);
}
}  // extern "C"
