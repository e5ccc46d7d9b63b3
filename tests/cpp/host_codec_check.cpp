// Stand-alone check of the host codecs (lz77-sss_amd/csrc/host_codec.cpp, linked directly):
// decode and extract of a hand-built stream, byte for byte, and the invalid streams of
// tests/test_extract_host.py::test_extract_rejects_invalid and
// tests/test_capi.py::test_decode_rejects_invalid_stream.  Built with the host sanitizers by
// tests/test_host_codec.py; exit status 0 = every check held.
#include "lz77sss.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                     \
        }                                                                   \
    } while (0)

static int decode(const std::vector<lz77sss_factor32>& F, uint8_t* out, uint64_t n) {
    return lz77sss_decode_u32(F.data(), F.size(), out, n);
}
static int decode(const std::vector<lz77sss_factor64>& F, uint8_t* out, uint64_t n) {
    return lz77sss_decode_u64(F.data(), F.size(), out, n);
}
static int extract(const std::vector<lz77sss_factor32>& F, uint64_t n, uint64_t pos, uint64_t len, uint8_t* out) {
    return lz77sss_extract_u32(F.data(), F.size(), n, pos, len, out);
}
static int extract(const std::vector<lz77sss_factor64>& F, uint64_t n, uint64_t pos, uint64_t len, uint8_t* out) {
    return lz77sss_extract_u64(F.data(), F.size(), n, pos, len, out);
}

// EINVAL with a message
static bool rejected(int rc) { return rc == LZ77SSS_EINVAL && lz77sss_last_error()[0] != 0; }

template <class FACT>
static void check_width() {
    using P = decltype(FACT::src);
    // literals a b c, an ordinary copy of "ab", literal x, a self-overlapping copy (src = start - 1)
    const std::vector<FACT> F = {{'a', 0}, {'b', 0}, {'c', 0}, {0, 2}, {'x', 0}, {5, 6}};
    const std::string T = "abcabxxxxxxx";
    const uint64_t n = T.size();
    // exact-size heap buffers: a byte written or read past the end is the sanitizer's to report
    std::vector<uint8_t> out(n);
    CHECK(decode(F, out.data(), n) == LZ77SSS_OK);
    CHECK(std::memcmp(out.data(), T.data(), n) == 0);
    for (uint64_t pos = 0; pos <= n; pos++)
        for (uint64_t len = 0; pos + len <= n; len++) {  // every range: pos = 0, across every factor boundary
            std::vector<uint8_t> part(len);
            CHECK(extract(F, n, pos, len, part.data()) == LZ77SSS_OK);
            CHECK(std::string(part.begin(), part.end()) == T.substr(pos, len));
        }
    CHECK(extract(F, n, n, 0, nullptr) == LZ77SSS_OK);  // len = 0 at pos = n
    CHECK(extract(std::vector<FACT>{}, 0, 0, 0, nullptr) == LZ77SSS_OK);
    CHECK(decode(std::vector<FACT>{}, nullptr, 0) == LZ77SSS_OK);

    // invalid_streams() of tests/decode_streams.py
    // (the sequential decode stops once n bytes are out: it rejects only the first two)
    struct bad { std::vector<FACT> F; uint64_t n; bool decode_too; };
    const std::vector<bad> B = {
        {{{97, 0}, {1, 2}}, 3, true},                                 // source not before start
        {{{97, 0}, {0, 2}}, 5, true},                                 // lengths fall short of n
        {{{97, 0}}, 0, false},                                        // nf > n (factors for an empty text)
        {{{97, 0}, {0, 4}, {0, (P)0xFFFFFFFFu}, {0, 1}}, 5, false},   // lengths overrun n
    };
    for (const bad& b : B) {
        std::vector<uint8_t> o(b.n);
        CHECK(rejected(extract(b.F, b.n, 0, b.n, o.data())));
        if (b.decode_too) CHECK(rejected(decode(b.F, o.data(), b.n)));
    }
    // test_decode_rejects_invalid_stream
    std::vector<uint8_t> o4(4), o3(3);
    CHECK(rejected(decode(std::vector<FACT>{{65, 0}, {5, 3}}, o4.data(), 4)));  // source 5 >= position 1
    CHECK(rejected(decode(std::vector<FACT>{{65, 0}}, o3.data(), 3)));          // stream shorter than n
    CHECK(rejected(decode(std::vector<FACT>{{65, 0}, {0, 5}}, o3.data(), 3)));  // a copy past n
    // ranges past the end of the text
    const uint64_t R[][2] = {{0, n + 1}, {n, 1}, {n + 1, 0}, {1ull << 63, 1ull << 63}, {~0ull, 2}};
    for (auto& r : R) CHECK(rejected(extract(F, n, r[0], r[1], out.data())));
    // NULL with a non-zero count
    CHECK(rejected(lz77sss_decode_u32(nullptr, 1, out.data(), 1)));
    CHECK(rejected(decode(F, nullptr, n)));
    CHECK(rejected(lz77sss_extract_u64(nullptr, 1, 1, 0, 1, out.data())));
    CHECK(rejected(extract(F, n, 0, 1, nullptr)));
}

int main() {
    check_width<lz77sss_factor32>();
    check_width<lz77sss_factor64>();
    if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
    return failures ? 1 : 0;
}
