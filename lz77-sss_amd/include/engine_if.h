// engine_if.h -- the C-ABI's only view of an engine, for both position widths.  The pipeline
// sources are compiled twice (namespace lz with pos_t = uint32_t, lz64 with -DLZ_POS64), and
// each compilation of csrc/engine.hip implements this interface; the C-ABI (csrc/capi.hip) is
// built once against it.  Pointers whose element type is pos_t travel as void*; pos_bytes()
// tells the few callers that care.
#pragma once
#include "../../include/lz77sss.h"
#include "lz77sss_internal.h"
#include "timer.h"

#include <memory>
#include <vector>

namespace lz {

// what the operations that exist only with pos_t = uint32_t answer on a 64-bit session
[[noreturn]] inline void not_on_pos64(const char* what) {
    throw error(LZ77SSS_EINVAL, std::string(what) + " is not available on a pos_t = uint64_t session");
}

struct engine_if {
    virtual ~engine_if() = default;
    virtual u32 pos_bytes() const = 0;       // sizeof(pos_t): 4 or 8
    virtual int device() const = 0;
    virtual u64 n() const = 0;
    virtual u64 max_n() const = 0;
    virtual u8* text() = 0;                  // HBM text (n + TEXT_PAD bytes)
    virtual hipStream_t stream() = 0;
    virtual void set_n(u64 n) = 0;
    virtual void load(const u8* t, u64 n) = 0;
    virtual u64 factorize(int phr_mode, u32 rk_seed, int log2_override, bool log, int fact_mode) = 0;
    virtual u64 num_fact() const = 0;
    virtual const void* factors() const = 0;  // device, (src, len) pairs of pos_t
    virtual void* factors_buf(u64 nf) = 0;    // device buffer for nf factors (decode input)
    virtual u64 decode(const void* F, u64 nf, u64 n_out, u8* d_out, bool cmp_with_text) = 0;
    virtual u8* dec_out(u64 n) = 0;
    virtual u64 verify(u64* first_bad) = 0;  // the factors against the loaded text (csrc/decode.hip)
    // csrc/decode_win.hip: the windowed decode, and bytes [pos, pos + len) of the text (device
    // bytes; info = path, largest hop count); check_verifiable as lz77sss_session_verify
    virtual void check_verifiable() const = 0;
    virtual u64 decode_windowed(const void* F, u64 nf, u64 n_out, u64 window, u8* d_out, bool cmp_with_text) = 0;
    virtual const u8* extract(const void* F, u64 nf, u64 n_tot, u64 pos, u64 len, bool cmp_with_text, u64* mism,
                              u64* info) = 0;
    virtual void sss(u64* size, int* has_runs) = 0;
    virtual u64 sss_size() const = 0;
    virtual const void* sss_ptr() const = 0;  // pos_t positions
    // sync set of a decision range (build_sss_range), kept apart from the text's own S: 64-bit
    // positions on both widths
    virtual void sss_range(u64 first, u64 end, u64 base, u64 window, u64* size, int* has_runs) = 0;
    virtual u64 range_size() const = 0;
    virtual const u64* range_ptr() const = 0;
    virtual u64 num_phr() const = 0;
    virtual const void* lpf_ptr() const = 0;  // (beg, end, src) triples of pos_t
    virtual const u32* sa_ptr() const = 0;
    virtual const u32* lcp_ptr() const = 0;
    virtual std::vector<u64>& stats() = 0;
    virtual phase_timer& timer() = 0;
    virtual double sss_kernel_ms() const = 0;
    virtual u64 sss_kernel_bytes() const = 0;
    virtual u32 dec_rounds() const = 0;
    // sharded factorization (rank-ordered greedy blocks); S_any: host or device
    virtual void set_sss(const u64* S_any, u64 count, bool runs) = 0;
    virtual u64 prepare(int phr_mode, bool external_sss, int log2_override) = 0;  // returns carried-table bytes
    virtual void* carried_table() = 0;
    virtual u64 carried_bytes() const = 0;   // capacity of the carried table
    virtual u64 greedy_block(u32 rk_seed, int log2_override, u64* state /* start, idxpos, zmask, carried, end,
                                                                        exit_start, exit_idxpos, exit_zmask */) = 0;
    virtual void spec_begin(int part, u64 base) = 0;
    virtual int spec_resolve(const void* true_tab, u64 bytes, int parts) = 0;
    // pos_t = uint32_t only (exact modes, containers); the containers return their size, the
    // bytes are at *_out()
    virtual u64 factorize_exact(bool) { not_on_pos64("session_factorize_exact"); }
    virtual u64 factorize_exact_smpl(int, int, u32, int, bool) { not_on_pos64("session_factorize_exact"); }
    virtual int last_fact_mode() const { not_on_pos64("last_fact_mode"); }
    virtual u64 huffman_container() { not_on_pos64("huffman"); }
    virtual const u8* huffman_out() const { not_on_pos64("huffman"); }
    virtual u64 ssszip_gapped() { not_on_pos64("ssszip_gapped"); }
    virtual const u8* ssszip_out() const { not_on_pos64("ssszip_gapped"); }
};

// each defined in its compilation of csrc/engine.hip; they throw lz::error
std::unique_ptr<engine_if> make_engine(int dev, u64 maxn);

}  // namespace lz
namespace lz64 {
std::unique_ptr<lz::engine_if> make_engine(int dev, lz::u64 maxn);
}  // namespace lz64
