// engine.hip -- engine lifetime and phase orchestration, compiled once per position width, and
// the engine_if implementation through which the C-ABI (csrc/capi.hip) drives it.  The
// orchestration mirrors factorizer::factorize / compute_approximation
// (include/lz77_sss/lz77_sss.hpp:285-491) for fact_mode = greedy, phr_mode = lpf_opt, p = 1.
#include "../../include/lz77sss.h"
#include "../include/engine.h"
#include "../include/engine_if.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <chrono>
#include <memory>
#include <string>

namespace LZ_NS {

void engine::init(int dev, u64 maxn) {
    device = dev;
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0) throw error(LZ77SSS_ENODEV, "no HIP device available");
    if (dev < 0 || dev >= cnt) throw error(LZ77SSS_EINVAL, "invalid device ordinal");
    LZ_HIP(hipSetDevice(dev));
    hipDeviceProp_t prop;
    LZ_HIP(hipGetDeviceProperties(&prop, dev));
    if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
        throw error(LZ77SSS_ENODEV, std::string("device is not gfx950: ") + prop.gcnArchName);
    LZ_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    max_n = maxn;
    LZ_HIP(hipMalloc(&d_text, max_n + TEXT_PAD));
    LZ_HIP(hipMemsetAsync(d_text, 0, max_n + TEXT_PAD, st));
    LZ_HIP(hipHostMalloc(&h_pin, 256, hipHostMallocDefault));
    for (auto& e : ev_pin) LZ_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    LZ_HIP(hipStreamSynchronize(st));
}

void engine::load(const u8* h_text, u64 n_) {
    if (n_ > max_n) throw error(LZ77SSS_EINVAL, "text larger than the session capacity");
    LZ_HIP(hipSetDevice(device));
    n = n_;
    runs_valid = false;
    brk_valid = false;
    if (n) LZ_HIP(hipMemcpyAsync(d_text, h_text, n, hipMemcpyHostToDevice, st));
    LZ_HIP(hipMemsetAsync(d_text + n, 0, TEXT_PAD, st));
    LZ_HIP(hipStreamSynchronize(st));
}

void engine::destroy() {
    for (hipEvent_t* e : {&sss_ev0, &sss_ev1, &sss_evA, &sss_evB}) {
        if (*e) (void)hipEventDestroy(*e);
        *e = nullptr;
    }
    if (d_text) (void)hipFree(d_text);
    if (d_text_rev) (void)hipFree(d_text_rev);
    d_text = d_text_rev = nullptr;
    if (h_pin) (void)hipHostFree(h_pin);
    h_pin = nullptr;
    for (auto& e : ev_pin)
        if (e) (void)hipEventDestroy(e), e = nullptr;
    if (st) (void)hipStreamDestroy(st);
    st = nullptr;
}

// fact_mode = skip_phrases: the gapped stream of factorize_skip_gaps
// (approximate/factorize/skip_gaps.cpp:31-61): {beg of the first phrase, 0}, then
// per phrase {src, len} followed by {gap length, 0} when the next phrase (or the
// sentinel {n, n+1, 0}) starts after its end
struct fill_batch {
    u8* p[engine::FILL_MAX];
    u64 bytes[engine::FILL_MAX];
    u32 pat[engine::FILL_MAX];
};
// blockIdx.y = the fill; 32-bit stores over the aligned words, then the tail bytes
__global__ void k_fills(fill_batch B) {
    const u32 f = blockIdx.y;
    u8* p = B.p[f];
    const u64 nb = B.bytes[f];
    const u32 pat = B.pat[f];
    const u64 head = ((4 - ((uintptr_t)p & 3)) & 3) < nb ? ((4 - ((uintptr_t)p & 3)) & 3) : nb;
    const u64 nw = (nb - head) / 4;
    const u64 t0 = (u64)blockIdx.x * blockDim.x + threadIdx.x, str = (u64)gridDim.x * blockDim.x;
    u32* w = (u32*)(p + head);
    const u32 rot = 8 * (u32)(((uintptr_t)p + head) & 3);  // (0: the words are aligned)
    const u32 wp = rot ? (pat >> rot) | (pat << (32 - rot)) : pat;
    for (u64 k = t0; k < nw; k += str) w[k] = wp;
    if (t0 < head) p[t0] = (u8)(pat >> (8 * ((uintptr_t)(p + t0) & 3)));
    const u64 tail0 = head + 4 * nw;
    if (t0 < nb - tail0) p[tail0 + t0] = (u8)(pat >> (8 * ((uintptr_t)(p + tail0 + t0) & 3)));
}
void engine::fills(std::initializer_list<fill_op> ops) {
    fill_batch B{};
    u32 nf = 0;
    u64 wmax = 0;
    for (const fill_op& o : ops) {
        if (!o.bytes || !o.p) continue;
        if (nf == (u32)FILL_MAX) throw error(LZ77SSS_EINTERNAL, "fills: too many");
        B.p[nf] = (u8*)o.p;
        B.bytes[nf] = o.bytes;
        B.pat[nf] = o.pat;
        wmax = std::max<u64>(wmax, o.bytes / 4 + 4);
        nf++;
    }
    if (!nf) return;
    const u32 gx = (u32)std::min<u64>(std::max<u64>(1, cdiv(wmax, 256)), 2048);
    k_fills<<<dim3(gx, nf), 256, 0, st>>>(B);
    LZ_HIP(hipGetLastError());
}

__global__ void k_skip_counts(const pos_t* __restrict__ P, u32 m, u32* __restrict__ cnt) {
    const u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (k > m) return;
    cnt[k] = k == m ? 1u : 1u + (P[3 * (k + 1)] > P[3 * k + 1] ? 1u : 0u);  // slot m: the leading gap record
}
__global__ void k_skip_write(const pos_t* __restrict__ P, u32 m, const u32* __restrict__ off, pos_t* __restrict__ F) {
    const u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (k > m) return;
    if (k == m) {
        F[0] = P[0];  // beg of the first phrase (or n: the sentinel)
        F[1] = 0;
        return;
    }
    const u64 o = 1 + off[k];
    const pos_t beg = P[3 * k], end = P[3 * k + 1], src = P[3 * k + 2], nb = P[3 * (k + 1)];
    F[2 * o] = src;
    F[2 * o + 1] = end - beg;
    if (nb > end) {
        F[2 * o + 2] = nb - end;
        F[2 * o + 3] = 0;
    }
}
u64 engine::emit_skip_phrases() {
    const u32 m = num_phr;
    pos_t* P = lpf.get((u64)(m + 1) * 3);
    const pos_t sent[3] = {(pos_t)n, (pos_t)n + 1, 0};
    LZ_HIP(hipMemcpyAsync(P + 3 * (u64)m, sent, sizeof(sent), hipMemcpyHostToDevice, st));
    LZ_HIP(hipStreamSynchronize(st));  // sent is a stack array
    u32* cnt = u32a.get((u64)m + 2);
    u32* off = u32b.get((u64)m + 2);
    k_skip_counts<<<cdiv((u64)m + 1, 256), 256, 0, st>>>(P, m, cnt);
    size_t tb = 0;
    LZ_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, cnt, off, (int)(m + 1), st));
    u8* t = scan_tmp.get(tb);
    LZ_HIP(hipcub::DeviceScan::ExclusiveSum(t, tb, cnt, off, (int)(m + 1), st));
    const u32 last = rd1(off + m, st);  // records of the m phrases (slot m is the leading record)
    const u64 z = (u64)last + 1;
    pos_t* F = fact.get(2 * z + 2);
    k_skip_write<<<cdiv((u64)m + 1, 256), 256, 0, st>>>(P, m, off, F);
    LZ_HIP(hipGetLastError());
    return z;
}

void engine::prepare_phrases(int phr_mode, bool external_sss) {
    const bool dbg = debug_enabled();
    const char* lean_env = std::getenv("LZ77SSS_LEAN");
    const bool lean_mode = lean_env ? lean_env[0] != '0' : n >= (1ull << 33);
    lean = lean_mode;
    if (lean_mode) {
        release_greedy_buffers();  // the last call's emitter buffers go before the phases grow
        timer.mark("release");     // (the phases after it report peaks without those buffers)
    }
    phr_info.valid = false;
    if (std::getenv("LZ77SSS_LCE_DEBUG") && !lce_dbg) {
        LZ_HIP(hipMalloc(&lce_dbg, 8 * sizeof(unsigned long long)));
        LZ_HIP(hipMemset(lce_dbg, 0, 8 * sizeof(unsigned long long)));
    }
    auto trace = [&](const char* what) {
        if (!dbg) return;
        LZ_HIP(hipStreamSynchronize(st));
        std::fprintf(stderr, "[lz77sss-debug] done %s (|S|=%u phrases=%u)\n", what, s, num_phr);
        if (lce_dbg) {
            unsigned long long c[8];
            LZ_HIP(hipMemcpy(c, lce_dbg, sizeof(c), hipMemcpyDeviceToHost));
            LZ_HIP(hipMemset(lce_dbg, 0, sizeof(c)));
            std::fprintf(stderr, "[lz77sss-debug]   lce fwd calls=%llu steps=%llu skips=%llu exact=%llu max_steps=%llu | bwd calls=%llu steps=%llu skips=%llu\n",
                         c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7]);
        }
    };
    if (phr_mode == LZ77SSS_LPF_OPT || phr_mode == LZ77SSS_LPF_NAIVE) {
        if (external_sss) {
            build_q_runs(d_text);  // the LCE's run table; S came from set_sss
        } else {
            build_sss(d_text);
        }
        timer.mark("sss");
        trace("sss");
        build_sa_s(d_text);
        timer.mark("sa_s");
        trace("sa_s");
        build_lcp_rmq(d_text);
        timer.mark("lcp_rmq");
        trace("lcp_rmq");
        if (std::getenv("LZ77SSS_DEBUG_VERIFY")) debug_verify_lce("sa_s + lcp");
        if (phr_mode == LZ77SSS_LPF_OPT) build_lpf_opt(d_text);
        else build_lpf_naive(d_text);
        timer.mark("lpf");
        trace("lpf");
        if (std::getenv("LZ77SSS_DEBUG_VERIFY")) debug_verify_phrases("lpf");
    } else {
        if (external_sss) throw error(LZ77SSS_EINVAL, "an external sync set needs phr_mode lpf_opt or lpf_naive");
        build_lpf_lnf(phr_mode == LZ77SSS_LPF_LNF_OPT ? 1 : 0);
        trace("lpf_lnf");
    }
    // large texts: the phases' own scratch goes back before the emitter allocates its base set
    // (grow-only buffers otherwise keep every phase's peak: 2.5 GiB of 288 GiB were left free
    // after a 50 GiB factorization in round 4).  Small texts keep them for the next call.
    if (lean_mode) release_phase_scratch();
}

// the emitter's buffers of the last call (lean mode, before the phases of the next one grow)
void engine::release_greedy_buffers() {
    fact.release(); tmp_greedy.release(); chunk_buf.release(); chunk_buf2.release(); rem_buf.release();
    add_keys32.release(); add_pos.release(); dirty_in.release(); dirty_out.release(); dirty_sorted.release();
    tmp_greedy2.release(); add_keys.release(); add_keys2.release();
    irank.release(); ekeys.release();
    evals.release(); ekeys2.release(); evals2.release(); occ_buf.release(); ist.release(); iend.release();
    ipos_buf.release(); iposr_buf.release(); tail_ins_buf.release(); seg_offs.release();
    g_sin.release(); g_sout.release(); g_valid.release(); g_cs.release(); g_tailc.release();
    g_succ.release(); g_seg_at.release(); g_ids.release(); g_chain.release(); g_dist[0].release(); g_dist[1].release();
    g_cbv.release(); g_bmI.release(); g_bmI2.release(); g_bmIb.release(); g_bmT.release();
    g_tmp1.release(); g_tmp2.release(); g_tmp3.release(); g_tmp4.release(); g_tmp5.release(); g_tmp6.release();
    g_tmp7.release(); g_tmp8.release(); g_ark.release(); g_ast.release(); g_aen.release(); g_offs.release();
    g_predk.release(); g_wk.release(); g_ids2.release(); g_brev.release(); g_bsum.release(); g_bincl.release();
    g_pbtmp.release(); g_pbcur.release(); g_pbm.release(); g_pwp.release(); g_pcnt.release(); g_sdk.release();
    g_dstart.release(); g_pflag.release(); g_bstart.release(); g_abeg.release(); g_abeg2.release(); g_bmA.release();
    g_x32.release(); g_xpos.release(); g_stash.release(); g_H.release(); g_Hs.release(); g_hsused.release();
    g_hsave.release(); g_htrue.release(); g_specbad.release(); fact_acc.release(); g_cut.release();
    g_xk.release(); g_xk2.release(); g_ls_h.release(); g_ls_g.release(); g_lng.release(); g_pbw.release();
    num_fact = 0;  // (the factors went with fact; the callers set last_fact_mode when they write new ones)
    negpow_key = {};  // the influence tables lived in tmp_greedy
    negpow_dev = nullptr;
    seg_at_clean = false;
    seg_at_n = 0;
}

// the buffers the phases before the emitter use only while they run: the SSS pass's stripe
// outputs, filter words, tile lists and run-record inputs, SA_S's rank levels and sort scratch,
// LPF's sparse tables over SA, PSV/NSV, candidates and pointer-doubling levels, the shared scratch.  Kept: the text, S, SA / ISA / LCP and its RMQ
// levels, the successor table, the run tables and block records (the LCE's view), the phrases.
void engine::release_phase_scratch() {
    lane_out.release(); lane_cnt.release(); lane_flag.release(); sss_ovf.release();
    sss_hitw.release(); sss_tflag.release(); sss_tiles.release(); sss_sflag.release(); sss_slist.release();
    sss_fcnt.release(); sss_tot.release(); q_info.release();
    blk_p.release(); blk_fo.release(); blk_lo.release(); blk_mk.release(); blk_ser.release(); blk_ss.release();
    run_scan_a.release(); run_scan_b.release(); S64.release(); s64 = 0;
    for (auto& b : rank_lv) b.release();
    nlev_rank = 0;
    for (auto& b : sa_min) b.release();
    for (auto& b : jump) b.release();  // (the emitter's segment linking grows its own levels again)
    PSV.release(); NSV.release(); cand.release(); p_Em.release(); p_lst.release(); p_ph3.release();
    key_len.release(); sa_tmp1.release(); sa_tmp2.release(); sa_tmp3.release();
    tmp_bytes.release(); tmp_bytes2.release(); tmp_bytes3.release(); scan_tmp.release();
    u64a.release(); u64b.release(); u32a.release(); u32b.release(); u32c.release(); u32d.release(); u32e.release();
    stats_released_scratch++;
}

// a sharded run gathers its sync set as 64-bit positions: pos_t = uint32_t
// narrows them on the device
#ifndef LZ_POS64
__global__ void k_narrow_u32(const u64* __restrict__ in, u64 m, u32* __restrict__ out) {
    const u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < m) out[k] = (u32)in[k];
}
#endif
void engine::set_sss(const u64* S_any, u64 count, bool runs) {
    LZ_HIP(hipSetDevice(device));
#ifndef LZ_POS64
    if (count && n > POS_MAX_N) throw error(LZ77SSS_EINVAL, "n too large for pos_t = uint32_t");
    u64* wide = u64a.get(count + 1);
    if (count) LZ_HIP(hipMemcpyAsync(wide, S_any, count * 8, hipMemcpyDefault, st));
    u32* src = u32e.get(count + 1);
    if (count) k_narrow_u32<<<cdiv(count, 256), 256, 0, st>>>(wide, count, src);
    LZ_HIP(hipStreamSynchronize(st));
#else
    const u64* src = S_any;
#endif
    // the same bound as build_sss: SA_S / LPF pass item counts to hipcub / rocprim as int
    if (count >= 0x7FFFFFFFull) throw error(LZ77SSS_EINVAL, "sync set too large");
    pos_t* d = S.get(count + 1);
    if (count) LZ_HIP(hipMemcpyAsync(d, src, count * sizeof(pos_t), hipMemcpyDefault, st));
    LZ_HIP(hipStreamSynchronize(st));
    s = (u32)count;
    has_runs = runs;
}

u64 engine::factorize(int phr_mode, u32 rk_seed, int log2_override, bool log, int fact_mode) {
    LZ_HIP(hipSetDevice(device));
    if (phr_mode < LZ77SSS_LPF_NAIVE || phr_mode > LZ77SSS_LPF_LNF_OPT) throw error(LZ77SSS_EINVAL, "unsupported phrase mode");
    if (n > POS_MAX_N)
        throw error(LZ77SSS_EINVAL, sizeof(pos_t) == 4 ? "n too large for pos_t = uint32_t" : "n too large");
    num_fact = 0;
    last_fact_mode = fact_mode;
    reset_stats();
    if (n == 0) return 0;
    const auto t_start = std::chrono::steady_clock::now();
    const u64 peak0 = g_dev_bytes.load();
    if (log) g_dev_peak.store(peak0);
    timer.begin(st);
    prepare_phrases(phr_mode, false);
    if (fact_mode == LZ77SSS_SKIP_PHRASES) {
        num_fact = emit_skip_phrases();
        timer.mark("skip_phrases");
    } else {
        num_fact = factorize_greedy(d_text, rk_seed, log2_override);
        timer.mark("greedy");
    }
    if (std::getenv("LZ77SSS_DEBUG_VERIFY") && fact_mode != LZ77SSS_SKIP_PHRASES) {
        u64 first = 0;
        const u64 bad = verify_factors(fact.p, num_fact, n, d_text, &first);
        std::fprintf(stderr, "[lz77sss-verify] factors: z=%llu bad positions=%llu first=%llu\n",
                     (unsigned long long)num_fact, (unsigned long long)bad, (unsigned long long)first);
    }
    if (debug_enabled()) std::fprintf(stderr, "[lz77sss-debug] done greedy (|S|=%u phrases=%u)\n", s, num_phr);
    stream_wait(st);
    if (log) {
        for (auto& [name, ms] : timer.read()) std::fprintf(stderr, "[lz77sss] %-10s %9.3f ms\n", name.c_str(), ms);
        std::fprintf(stderr, "[lz77sss] n=%llu |S|=%u phrases=%u factors=%llu outer=%llu rounds=%llu\n",
                     (unsigned long long)n, s, num_phr, (unsigned long long)num_fact,
                     (unsigned long long)stats[12], (unsigned long long)stats[13]);
        if (fact_mode != LZ77SSS_SKIP_PHRASES) log_summary(t_start);
    }
    return num_fact;
}

// the summary a logged factorization prints (lz77_sss.hpp:345-353, formats of
// misc/utils.hpp:54-96); peak memory = the session's peak device bytes + n (the text)
static std::string fmt_time(u64 ns) {
    if (ns > 10000000000ull) return std::to_string(ns / 1000000000) + " s";
    if (ns > 10000000ull) return std::to_string(ns / 1000000) + " ms";
    if (ns > 10000ull) return std::to_string(ns / 1000) + " us";
    return std::to_string(ns) + " ns";
}
static std::string fmt_size(u64 B) {
    if (B > 10000000000ull) return std::to_string(B / 1000000000) + " GB";
    if (B > 10000000ull) return std::to_string(B / 1000000) + " MB";
    if (B > 10000ull) return std::to_string(B / 1000) + " KB";
    return std::to_string(B) + " B";
}
void engine::log_summary(std::chrono::steady_clock::time_point t_start) const {
    const u64 ns = (u64)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_start).count();
    const double comp_ratio = n / (double)std::max<u64>(1, num_fact);
    const double tp = 1000.0 * (double)n / (double)std::max<u64>(1, ns);
    std::printf("num. of factors: %llu\n", (unsigned long long)num_fact);
    std::printf("input length / num. of factors: %s\n", std::to_string(comp_ratio).c_str());
    std::printf("total time: %s\n", fmt_time(ns).c_str());
    std::printf("throughput: %s MB/s\n", std::to_string(tp).c_str());
    std::printf("peak memory consumption: %s\n", fmt_size(g_dev_peak.load() + n).c_str());
    std::fflush(stdout);
}

// ===========================================================================
// this width's engine behind the C-ABI (engine_if.h)
// ===========================================================================
namespace {
struct engine_impl final : lz::engine_if {
    engine E;
    ~engine_impl() override { E.destroy(); }
    u32 pos_bytes() const override { return sizeof(pos_t); }
    int device() const override { return E.device; }
    u64 n() const override { return E.n; }
    u64 max_n() const override { return E.max_n; }
    u8* text() override { return E.d_text; }
    hipStream_t stream() override { return E.st; }
    void set_n(u64 n) override { E.n = n; }
    void load(const u8* t, u64 n) override { E.load(t, n); }
    u64 factorize(int phr, u32 seed, int log2, bool log, int fact_mode) override {
        return E.factorize(phr, seed, log2, log, fact_mode);
    }
    u64 num_fact() const override { return E.num_fact; }
    const void* factors() const override { return E.fact.p; }
    void* factors_buf(u64 nf) override { return E.fact.get(2 * nf + 2); }
    u64 decode(const void* F, u64 nf, u64 n_out, u8* d_out, bool cmp) override {
        return E.decode_device((const pos_t*)F, nf, n_out, d_out, cmp ? E.d_text : nullptr);
    }
    u8* dec_out(u64 n) override { return E.dec_out.get(n); }
    u64 verify(u64* first_bad) override {
        const u64 bad = E.verify_factors(E.fact.p, E.num_fact, E.n, E.d_text, first_bad);
        LZ_HIP(hipStreamSynchronize(E.st));
        return bad;
    }
    void check_verifiable() const override { E.check_verifiable(); }
    u64 decode_windowed(const void* F, u64 nf, u64 n_out, u64 window, u8* d_out, bool cmp) override {
        return E.decode_windowed((const pos_t*)F, nf, n_out, window, d_out, cmp ? E.d_text : nullptr);
    }
    const u8* extract(const void* F, u64 nf, u64 n_tot, u64 pos, u64 len, bool cmp, u64* mism, u64* info) override {
        return E.extract_device((const pos_t*)F, nf, n_tot, pos, len, cmp ? E.d_text : nullptr, mism, info);
    }
    void sss(u64* size, int* has_runs) override {
        LZ_HIP(hipSetDevice(E.device));
        E.build_sss(E.d_text);
        LZ_HIP(hipStreamSynchronize(E.st));
        *size = E.s;
        *has_runs = E.has_runs;
    }
    u64 sss_size() const override { return E.s; }
    const void* sss_ptr() const override { return E.S.p; }
    void sss_range(u64 first, u64 end, u64 base, u64 window, u64* size, int* has_runs) override {
        LZ_HIP(hipSetDevice(E.device));
        E.build_sss_range(first, end, base, window);
        *size = E.s64;
        *has_runs = E.has_runs64;
    }
    u64 range_size() const override { return E.s64; }
    const u64* range_ptr() const override { return E.S64.p; }
    u64 num_phr() const override { return E.num_phr; }
    const void* lpf_ptr() const override { return E.lpf.p; }
    const u32* sa_ptr() const override { return E.SA.p; }
    const u32* lcp_ptr() const override { return E.lcp_rmq[0].p; }
    std::vector<u64>& stats() override { return E.stats; }
    lz::phase_timer& timer() override { return E.timer; }
    double sss_kernel_ms() const override { return E.sss_ms(); }
    u64 sss_kernel_bytes() const override { return E.sss_kernel_bytes; }
    u32 dec_rounds() const override { return E.dec_rounds; }
    void set_sss(const u64* S_any, u64 count, bool runs) override { E.set_sss(S_any, count, runs); }
    // the two halves of lz77sss_session_prepare / _greedy_block (a block of a sharded run)
    u64 prepare(int phr_mode, bool external_sss, int log2_override) override {
        LZ_HIP(hipSetDevice(E.device));
        if (phr_mode != LZ77SSS_LPF_OPT && phr_mode != LZ77SSS_LPF_NAIVE)
            throw error(LZ77SSS_EINVAL, "a sharded factorization needs phr_mode lpf_opt or lpf_naive");
        if (E.n > POS_MAX_N) throw error(LZ77SSS_EINVAL, "n too large for pos_t");
        E.num_fact = 0;
        E.last_fact_mode = LZ77SSS_GREEDY;
        E.reset_stats();
        E.spec_track = false;
        E.timer.begin(E.st);
        E.prepare_phrases(phr_mode, external_sss);
        const u64 ent = E.n ? E.carried_entries(log2_override) : 1;
        E.g_Hs.get(ent);
        LZ_HIP(hipStreamSynchronize(E.st));
        return ent * sizeof(pos_t);
    }
    void* carried_table() override { return E.g_Hs.p; }
    u64 carried_bytes() const override { return E.g_Hs.cap * sizeof(pos_t); }
    u64 greedy_block(u32 rk_seed, int log2_override, u64* st) override {
        LZ_HIP(hipSetDevice(E.device));
        LZ_NS::greedy_block b;
        b.start = (pos_t)st[0];
        b.idxpos = (pos_t)st[1];
        b.zmask = (u32)st[2];
        b.carried = (st[3] & 1) != 0;
        b.seed = (st[3] & 2) != 0;
        b.end = (pos_t)st[4];
        E.timer.begin(E.st);
        E.last_fact_mode = LZ77SSS_GREEDY;
        E.num_fact = E.n ? E.factorize_greedy(E.d_text, rk_seed, log2_override, &b) : 0;
        E.timer.mark("greedy");
        LZ_HIP(hipStreamSynchronize(E.st));
        st[5] = b.exit_start;
        st[6] = b.exit_idxpos;
        st[7] = b.exit_zmask;
        return E.num_fact;
    }
    void spec_begin(int part, u64 base) override { E.spec_begin(part, base); }
    int spec_resolve(const void* true_tab, u64 bytes, int parts) override {
        return E.spec_resolve(true_tab, bytes, parts);
    }
#ifndef LZ_POS64  // (lz64::engine declares these and never defines them)
    u64 factorize_exact(bool log) override { return E.factorize_exact(log); }
    u64 factorize_exact_smpl(int transf_mode, int phr_mode, u32 rk_seed, int log2_override, bool log) override {
        return E.factorize_exact_smpl(transf_mode, phr_mode, rk_seed, log2_override, log);
    }
    int last_fact_mode() const override { return E.last_fact_mode; }
    u64 huffman_container() override { return E.huffman_container(); }
    const u8* huffman_out() const override { return E.hf_out.p; }
    u64 ssszip_gapped() override { return E.ssszip_gapped(); }
    const u8* ssszip_out() const override { return E.ssz_out.p; }
#endif
};
}  // namespace

std::unique_ptr<lz::engine_if> make_engine(int dev, u64 maxn) {
    auto p = std::make_unique<engine_impl>();
    p->E.init(dev, maxn);
    return p;
}

}  // namespace LZ_NS
