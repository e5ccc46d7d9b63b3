// host_codec.cpp -- the parts of the C-ABI (include/lz77sss.h) that run on the host alone: the
// sequential decode, the range extract, and the thread's last error message.  This is the code
// that parses untrusted factor streams on the CPU, so it depends on nothing but the public
// header and the standard library and compiles on its own (tests/cpp/host_codec_check.cpp links
// it under the host sanitizers).
#include "../../include/lz77sss.h"

#include <algorithm>
#include <exception>
#include <new>
#include <string>
#include <vector>

#define LZ77SSS_API __attribute__((visibility("default")))

static thread_local std::string g_err;

namespace lz {
// the message lz77sss_last_error returns on this thread (csrc/capi.hip reports through it)
void set_last_error(const char* msg) { g_err = msg; }
}  // namespace lz

static int invalid(const char* msg) {
    g_err = msg;
    return LZ77SSS_EINVAL;
}

// decode: algorithms/common.cpp:31-54 (sequential; forward byte copy allows overlap)
template <class FACT>
static int host_decode(const FACT* f, uint64_t nf, uint8_t* out, uint64_t n) {
    if ((!f && nf) || (!out && n)) return invalid("NULL argument");
    uint64_t pos = 0, k = 0;
    while (pos < n && k < nf) {
        const FACT x = f[k++];
        if (x.len == 0) {
            out[pos++] = (uint8_t)x.src;
        } else {
            if ((uint64_t)x.src >= pos || x.len > n - pos) return invalid("invalid factor during decode");
            for (uint64_t i = 0; i < x.len; i++) out[pos + i] = out[x.src + i];
            pos += x.len;
        }
    }
    if (pos != n) return invalid("factors do not cover the output length");
    return LZ77SSS_OK;
}

// range extract: a per-position walk over the prefix sum of the lengths.  A hop that lands
// inside the part of the range already written takes its byte from there
template <class FACT>
static int host_extract(const FACT* f, uint64_t nf, uint64_t n, uint64_t pos, uint64_t len, uint8_t* out) {
    if ((!f && nf) || (!out && len)) return invalid("NULL argument");
    if (pos > n || len > n - pos) return invalid("range past the end of the text");
    if (nf > n) return invalid("factor count does not fit the text length");
    std::vector<uint64_t> start;
    try {
        start.resize(nf + 1);
    } catch (const std::bad_alloc&) {
        g_err = "out of memory";
        return LZ77SSS_ENOMEM;
    } catch (const std::exception& e) {  // (a count past the vector's max_size)
        g_err = e.what();
        return LZ77SSS_EINTERNAL;
    }
    uint64_t at = 0;
    for (uint64_t k = 0; k < nf; k++) {
        start[k] = at;
        const uint64_t l = f[k].len ? (uint64_t)f[k].len : 1;
        if (at >= n || l > n - at) return invalid("factor lengths do not sum to n");
        if (f[k].len && (uint64_t)f[k].src >= at) return invalid("factor source not before its position");
        at += l;
    }
    start[nf] = at;
    if (at != n) return invalid("factor lengths do not sum to n");
    uint64_t k = 0;  // the factor of the last position looked up (neighbours share it)
    for (uint64_t i = 0; i < len; i++) {
        uint64_t p = pos + i;
        for (;;) {
            if (p >= pos && p < pos + i) {
                out[i] = out[p - pos];
                break;
            }
            if (p < start[k] || p >= start[k + 1])
                k = (uint64_t)(std::upper_bound(start.begin(), start.end() - 1, p) - start.begin()) - 1;
            if (f[k].len == 0) {
                out[i] = (uint8_t)f[k].src;
                break;
            }
            const uint64_t d = start[k] - f[k].src;
            uint64_t off = p - start[k];
            if (off >= d) off %= d;
            p = f[k].src + off;
        }
    }
    return LZ77SSS_OK;
}

extern "C" {

LZ77SSS_API const char* lz77sss_last_error(void) { return g_err.c_str(); }

LZ77SSS_API int lz77sss_decode_u32(const lz77sss_factor32* f, uint64_t nf, uint8_t* out, uint64_t n) {
    return host_decode(f, nf, out, n);
}
LZ77SSS_API int lz77sss_decode_u64(const lz77sss_factor64* f, uint64_t nf, uint8_t* out, uint64_t n) {
    return host_decode(f, nf, out, n);
}
LZ77SSS_API int lz77sss_extract_u32(const lz77sss_factor32* f, uint64_t nf, uint64_t n, uint64_t pos, uint64_t len,
                                    uint8_t* out) {
    return host_extract(f, nf, n, pos, len, out);
}
LZ77SSS_API int lz77sss_extract_u64(const lz77sss_factor64* f, uint64_t nf, uint64_t n, uint64_t pos, uint64_t len,
                                    uint8_t* out) {
    return host_extract(f, nf, n, pos, len, out);
}

}  // extern "C"
