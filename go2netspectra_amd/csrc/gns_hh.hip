// gns_hh.hip -- the device heavy-hitter list (gns_hh.hpp): its kernels, the
// list of one cell array (hh_heavy_list), id -> key bytes, and the canonical
// order of packed rows for the multi-GPU merge (gns_hh_order_rows).  No engine
// state: callers pass their dictionary, their cells and an HhScratch.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <sys/resource.h>
#include <vector>

#include "gns_common.hpp"
#include "gns_hh.hpp"
#include "gns_scan.cuh"

namespace gns {

// flow ids -> key bytes (GNS_ID_NONE -> zero bytes, the reference's reset FP)
__global__ __launch_bounds__(256) void k_ids_to_bytes(const uint32_t *ids, uint64_t n, DictDev D,
                                                      uint8_t *out) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const uint32_t id = ids[p];
    uint32_t r[12];
    if (id != GNS_ID_NONE) load_record(D, id, r);
    for (uint32_t j = 0; j < D.K; j++) {
        const uint32_t w = id != GNS_ID_NONE ? r[1 + (j >> 2)] : 0u;
        out[p * D.K + j] = (uint8_t)(w >> (8 * (j & 3)));
    }
}

// cells whose counter >= thr -> (value<<32 | id) candidate list
// kHhItems cells per lane; one global atomic per workgroup reserves the
// candidates' slots (a per-lane atomic on the one counter serialized every
// candidate: 0.59 ms per call at the bench geometry).  Order is irrelevant:
// the host dedupes and sorts.
constexpr uint32_t kHhItems = 8;
// Device-side heavy-hitter list (count_min.go:178-247 HeavyHitters), all
// hand-written (no library sort):
//   candidates   cells with value >= threshold (one global atomic per workgroup);
//   per-flow max every candidate atomicMax'es (epoch << 32 | value) into a dense
//                per-flow-id word, then the one candidate per flow that carries the
//                max and wins the flow's mark emits (id, max) -- the dedupe of
//                count_min.go:214-228's map, order-free, O(candidates);
//   order        a stable LSD radix sort of the unique entries (8-bit digits,
//                device-wide passes: block histograms, the K2 scan, stable
//                ballot-multisplit scatter) by the primary key (value desc, key
//                bytes 0..3); only when two entries tie on it (the same value and
//                the same first four key bytes) is the list re-sorted by the whole
//                key (bytes K-1..4 first, then the primary key).  A pass whose
//                digit is the same for every entry (IPv4 slots' zero padding) only
//                copies.  Canonical order: value desc, flow bytes asc.
// A candidate whose id is not a dictionary slot (a corrupt fingerprint word) is
// skipped and raises *bad: the host then fails the call with GNS_E_HIP instead of
// letting the per-flow words be indexed out of bounds.
__global__ __launch_bounds__(256) void k_hh_best(const uint64_t *cand, uint32_t n, unsigned long long *best,
                                                 uint32_t epoch, uint64_t slots, uint32_t *bad) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t c = cand[i];  // value << 32 | id
    if ((uint32_t)c >= slots) { atomicOr(bad, 1u); return; }
    atomicMax(&best[(uint32_t)c], (unsigned long long)epoch << 32 | (c >> 32));
}

__global__ __launch_bounds__(256) void k_hh_emit(const uint64_t *cand, uint32_t n, const unsigned long long *best,
                                                 uint32_t *mark, uint32_t epoch, uint64_t slots, uint32_t *uid,
                                                 uint32_t *uval, uint32_t *nu) {
    __shared__ uint32_t s_n, s_base;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    bool out = false;
    uint32_t id = 0, v = 0;
    if (i < n) {
        const uint64_t c = cand[i];
        id = (uint32_t)c;
        v = (uint32_t)(c >> 32);
        out = id < slots && (uint32_t)best[id] == v && atomicExch(&mark[id], epoch) != epoch;  // one per flow
    }
    const uint32_t off = out ? atomicAdd(&s_n, 1u) : 0u;
    __syncthreads();
    if (threadIdx.x == 0) s_base = s_n ? atomicAdd(nu, s_n) : 0u;
    __syncthreads();
    if (out) {
        uid[s_base + off] = id;
        uval[s_base + off] = v;
    }
}

// A heavy-hitter list on the device: entry e has flow bytes ub[e*stride .. +K) and
// a value, uval[e] -- or, for packed rows [flow | u32 value] (uval null), the
// little-endian word at ub[e*stride + K].
struct HhSrc {
    const uint32_t *uval;
    const uint8_t *ub;
    uint32_t K, stride;
};
__device__ __forceinline__ uint32_t hh_val(const HhSrc &h, uint32_t e) {
    if (h.uval) return h.uval[e];
    const uint8_t *q = h.ub + (uint64_t)e * h.stride + h.K;
    return (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
}
__device__ __forceinline__ uint32_t hh_byte(const HhSrc &h, uint32_t e, uint32_t b) {
    return b < h.K ? (uint32_t)h.ub[(uint64_t)e * h.stride + b] : 0u;
}

// One radix pass's digit of entry e: mode 0 = byte `b` of the value, inverted
// (descending); mode 1 = key byte b (0 beyond K).
struct RsDigit {
    uint32_t mode, b;
    HhSrc src;
};
__device__ __forceinline__ uint32_t rs_digit(const RsDigit &r, uint32_t e) {
    if (r.mode == 0) return 255u - ((hh_val(r.src, e) >> (8u * r.b)) & 255u);
    return hh_byte(r.src, e, r.b);
}

constexpr uint32_t kRsPer = 16;                 // entries per thread
constexpr uint32_t kRsBlock = 256 * kRsPer;     // entries per block of a pass

__global__ __launch_bounds__(256) void k_rs_hist(const uint32_t *perm, uint32_t n, RsDigit r, uint32_t *hist) {
    __shared__ uint32_t s_h[256];
    const uint32_t tid = threadIdx.x;
    s_h[tid] = 0;
    __syncthreads();
    const uint32_t beg = blockIdx.x * kRsBlock;
#pragma unroll 4
    for (uint32_t k = 0; k < kRsPer; k++) {
        const uint32_t j = beg + k * 256 + tid;
        if (j < n) atomicAdd(&s_h[rs_digit(r, perm[j])], 1u);
    }
    __syncthreads();
    hist[(uint64_t)blockIdx.x * 256 + tid] = s_h[tid];
}

// Stable scatter of one pass: entries of a block in (round, wave, lane) order =
// position order; per wave-instruction the lanes of one digit are found by
// eight ballots (no reliance on LDS-atomic lane order).  offs = the scanned
// block-major histogram (global start of every (block, digit) run); tot / total
// = the digit totals' exclusive scan: a digit holding every entry makes the pass
// a copy (the order cannot change).
__global__ __launch_bounds__(256) void k_rs_scatter(const uint32_t *perm, uint32_t n, RsDigit r, const uint32_t *offs,
                                                    const uint32_t *tot, const uint32_t *total, uint32_t *out) {
    __shared__ uint32_t s_base[256];
    __shared__ uint32_t s_wave[4][256];
    __shared__ uint32_t s_copy;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t beg = blockIdx.x * kRsBlock;
    if (tid == 0) {
        const uint32_t d0 = rs_digit(r, perm[0]);
        const uint32_t hi = d0 < 255u ? tot[d0 + 1] : *total;
        s_copy = hi - tot[d0] == n;
    }
    s_base[tid] = offs[(uint64_t)blockIdx.x * 256 + tid];
    __syncthreads();
    if (s_copy) {  // block-uniform
        for (uint32_t k = 0; k < kRsPer; k++) {
            const uint32_t j = beg + k * 256 + tid;
            if (j < n) out[j] = perm[j];
        }
        return;
    }
    const uint64_t lt = lane ? (~0ull >> (64u - lane)) : 0ull;
    for (uint32_t k = 0; k < kRsPer; k++) {
        if (beg + k * 256 >= n) break;  // block-uniform
        const uint32_t j = beg + k * 256 + tid;
        const bool valid = j < n;
        const uint32_t e = valid ? perm[j] : 0u;
        const uint32_t dg = valid ? rs_digit(r, e) : 0u;
        uint64_t peers = __ballot(valid);
#pragma unroll
        for (uint32_t bit = 0; bit < 8; bit++) {
            const uint64_t m = __ballot(valid && ((dg >> bit) & 1u));
            peers &= ((dg >> bit) & 1u) ? m : ~m;
        }
        s_wave[0][tid] = 0; s_wave[1][tid] = 0; s_wave[2][tid] = 0; s_wave[3][tid] = 0;
        __syncthreads();
        const uint32_t rank = (uint32_t)__popcll(peers & lt);
        if (valid && rank == 0) s_wave[wave][dg] = (uint32_t)__popcll(peers);
        __syncthreads();
        if (valid) {
            uint32_t pos = s_base[dg] + rank;
            for (uint32_t w = 0; w < wave; w++) pos += s_wave[w][dg];
            out[pos] = e;
        }
        __syncthreads();
        s_base[tid] += s_wave[0][tid] + s_wave[1][tid] + s_wave[2][tid] + s_wave[3][tid];
        __syncthreads();
    }
}

// Whether two neighbours of the primary order tie on (value, key bytes 0..3):
// only then does the list need the whole-key order.
__global__ __launch_bounds__(256) void k_hh_ties(const uint32_t *perm, uint32_t n, HhSrc h, uint32_t *flag) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x + 1;
    if (j >= n) return;
    const uint32_t a = perm[j - 1], b = perm[j];
    if (hh_val(h, a) != hh_val(h, b)) return;
    bool eq = true;
    for (uint32_t t = 0; t < 4 && t < h.K; t++) eq = eq && hh_byte(h, a, t) == hh_byte(h, b, t);
    if (eq) atomicOr(flag, 1u);
}

__global__ __launch_bounds__(256) void k_hh_iota(uint32_t *perm, uint32_t n) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j < n) perm[j] = j;
}

// ordered output: flow bytes and values in list order (one D2H each), or packed
// rows [flow | u32 value] (rows non-null: the multi-GPU exchange keeps them on the device)
__global__ __launch_bounds__(256) void k_hh_gather(const uint32_t *perm, HhSrc h, uint32_t n, uint8_t *ob,
                                                   uint32_t *ov, uint8_t *rows) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const uint32_t u = perm[j], K = h.K;
    const uint32_t v = hh_val(h, u);
    if (rows) {
        uint8_t *o = rows + (uint64_t)j * (K + 4);
        for (uint32_t t = 0; t < K; t++) o[t] = hh_byte(h, u, t);
        o[K] = (uint8_t)v; o[K + 1] = (uint8_t)(v >> 8); o[K + 2] = (uint8_t)(v >> 16); o[K + 3] = (uint8_t)(v >> 24);
        return;
    }
    for (uint32_t t = 0; t < K; t++) ob[(uint64_t)j * K + t] = hh_byte(h, u, t);
    ov[j] = v;
}

__global__ __launch_bounds__(256) void k_hh_candidates(const uint32_t *val, const uint32_t *fp,
                                                       uint64_t cells, uint32_t thr,
                                                       uint64_t *cand, uint32_t *ncand, uint32_t cap) {
    __shared__ uint32_t s_n, s_base;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const uint64_t c0 = (uint64_t)blockIdx.x * 256 * kHhItems + threadIdx.x;
    uint64_t cv[kHhItems];
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t i = 0; i < kHhItems; i++) {
        const uint64_t c = c0 + (uint64_t)i * 256;
        cv[i] = 0;
        if (c < cells) {
            const uint32_t v = val[c];
            if (v > 0 && v >= thr) { cv[i] = (uint64_t)v << 32 | fp[c]; cnt++; }
        }
    }
    const uint32_t off = cnt ? atomicAdd(&s_n, cnt) : 0u;
    __syncthreads();
    if (threadIdx.x == 0) s_base = s_n ? atomicAdd(ncand, s_n) : 0u;
    __syncthreads();
    uint32_t q = s_base + off;
#pragma unroll
    for (uint32_t i = 0; i < kHhItems; i++)
        if (cv[i]) { if (q < cap) cand[q] = cv[i]; q++; }
}

__global__ void k_fill_u32(uint32_t *p, uint64_t n, uint32_t v) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        p[i] = v;
}

}  // namespace gns

// ===========================================================================
// Host side
// ===========================================================================
namespace gns {

void HhScratch::free_all() {
    dfree(obytes); obytes = nullptr; obytes_n = 0;
    if (hpin) (void)hipHostFree(hpin);
    hpin = nullptr; hpin_n = 0;
    if (hsm) (void)hipHostFree(hsm);
    hsm = nullptr;
    dfree(cand); dfree(ncand); dfree(bytes);
    dfree(best); dfree(mark); dfree(u32a); dfree(u32b); dfree(u32c); dfree(u32d); dfree(rsh);
    cand = nullptr; ncand = nullptr; bytes = nullptr;
    best = nullptr; mark = nullptr; u32a = u32b = u32c = u32d = nullptr; rsh = nullptr;
    cap = 0; bytes_n = 0;
    best_n = mark_n = u32a_n = u32b_n = u32c_n = u32d_n = rsh_n = 0; hh_epoch = 0;
}

// through the grow-only scratch when small (heavy-hitter lists), a temporary
// buffer for whole-state exports
int hh_ids_to_host_bytes(HhScratch &sc, hipStream_t st, const DictDev &D, const uint32_t *d_ids, uint64_t n,
                         uint8_t *host) {
    if (n == 0 || D.K == 0) return GNS_OK;
    const uint64_t nb = n * D.K;
    const bool tmp = nb > (64ull << 20);
    uint8_t *d = nullptr;
    if (tmp) GNS_TRY(dalloc(reinterpret_cast<void **>(&d), nb));
    else { GNS_TRY(grow_buf(&sc.bytes, sc.bytes_n, nb)); d = sc.bytes; }
    hipLaunchKernelGGL(k_ids_to_bytes, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_ids, n, D, d);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(host, d, nb, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (tmp) dfree(d);
    if (e != hipSuccess) { set_error("ids_to_bytes: %s", hipGetErrorString(e)); return GNS_E_HIP; }
    return GNS_OK;
}

int hh_ids_to_dev_bytes(hipStream_t st, const DictDev &D, const uint32_t *d_ids, uint64_t n, uint8_t *d_out) {
    if (n == 0 || D.K == 0) return GNS_OK;
    hipLaunchKernelGGL(k_ids_to_bytes, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_ids, n, D, d_out);
    GNS_HIP(hipGetLastError());
    return GNS_OK;
}

// HeavyHitters (count_min.go:178-247): a flow's max over its buckets reaches the
// threshold iff one of its buckets does, so only cells >= threshold are
// candidates; dedupe by fingerprint keeping the max; sort value desc.
// the per-flow-id words cover every slot of the dictionary (zeroed when (re)allocated:
// the epochs of the calls start at 1); bump: a new call's epoch
static int heavy_flow_words(HhScratch &sc, uint64_t slots, hipStream_t st, bool bump) {
    if (sc.best_n < slots || !sc.best || sc.mark_n < slots || !sc.mark) {
        dfree(sc.best); dfree(sc.mark);
        sc.best = nullptr; sc.mark = nullptr; sc.best_n = sc.mark_n = 0;
        GNS_TRY(dalloc(reinterpret_cast<void **>(&sc.best), slots * 8));
        GNS_TRY(dalloc(reinterpret_cast<void **>(&sc.mark), slots * 4));
        sc.best_n = sc.mark_n = slots;
        GNS_HIP(hipMemsetAsync(sc.best, 0, slots * 8, st));
        GNS_HIP(hipMemsetAsync(sc.mark, 0, slots * 4, st));
        sc.hh_epoch = 0;
    }
    if (bump && ++sc.hh_epoch == 0) {  // wrapped: clear, restart at 1
        GNS_HIP(hipMemsetAsync(sc.best, 0, sc.best_n * 8, st));
        GNS_HIP(hipMemsetAsync(sc.mark, 0, sc.mark_n * 4, st));
        sc.hh_epoch = 1;
    }
    return GNS_OK;
}

static int small_pin(HhScratch &sc) {
    if (!sc.hsm) GNS_HIP(hipHostMalloc(reinterpret_cast<void **>(&sc.hsm), 64, hipHostMallocDefault));
    return GNS_OK;
}

int hh_reserve(HhScratch &sc, uint64_t cells, uint64_t slots, uint32_t K, hipStream_t st) {
    GNS_TRY(heavy_flow_words(sc, slots, st, false));
    if (!sc.ncand) GNS_TRY(dalloc(reinterpret_cast<void **>(&sc.ncand), 16));
    if (!sc.cand) {
        const uint64_t want = std::min<uint64_t>(cells, 1ull << 22);
        GNS_TRY(dalloc(reinterpret_cast<void **>(&sc.cand), want * 8));
        sc.cap = want;
    }
    const uint64_t nu = std::min<uint64_t>(std::min(cells, slots), 1ull << 20);
    GNS_TRY(grow_buf(&sc.u32a, sc.u32a_n, nu / 2));
    GNS_TRY(grow_buf(&sc.u32b, sc.u32b_n, nu / 2 + 1));
    GNS_TRY(grow_buf(&sc.u32c, sc.u32c_n, nu));
    GNS_TRY(grow_buf(&sc.u32d, sc.u32d_n, nu / 2));
    GNS_TRY(grow_buf(&sc.bytes, sc.bytes_n, nu / 2 * std::max<uint32_t>(K, 1)));
    GNS_TRY(grow_buf(&sc.obytes, sc.obytes_n, nu / 2 * std::max<uint32_t>(K, 1)));
    if (!sc.hpin) {
        const uint64_t want = nu * (std::max<uint32_t>(K, 1) + 4);
        GNS_HIP(hipHostMalloc(reinterpret_cast<void **>(&sc.hpin), want, hipHostMallocDefault));
        sc.hpin_n = want;
    }
    // the order's pass histograms and the small pinned read-back words for nu entries too:
    // a window's first list then allocates nothing (an allocation inside one list call was
    // followed by an 18-36 ms dispatch stall of a LATER call, profiles/r06_hh_spikes.txt)
    const uint64_t nblk = (nu + kRsBlock - 1) / kRsBlock, ngrp = (nblk + kTGrp - 1) / kTGrp;
    GNS_TRY(grow_buf(&sc.rsh, sc.rsh_n, (nblk + ngrp + 1) * 256 + 4));
    return small_pin(sc);
}

// GNS_HH_TRACE=1: the heavy-hitter list's phases timed on stderr (each mark
// synchronizes the stream first; diagnostics only, never on by default).
struct HhTrace {
    bool on;
    hipStream_t st;
    std::chrono::steady_clock::time_point t;
    explicit HhTrace(hipStream_t s) : on(getenv("GNS_HH_TRACE") != nullptr), st(s), t(std::chrono::steady_clock::now()) {}
    void mark(const char *what, uint64_t n, bool sync = true) {
        if (!on) return;
        if (sync) (void)hipStreamSynchronize(st);
        const auto now = std::chrono::steady_clock::now();
        struct rusage ru;
        getrusage(RUSAGE_THREAD, &ru);
        fprintf(stderr, "[hh] %-12s n=%-9llu %8.3f ms  nivcsw=%ld nvcsw=%ld\n", what, (unsigned long long)n,
                std::chrono::duration<double, std::milli>(now - t).count(), ru.ru_nivcsw, ru.ru_nvcsw);
        t = now;
    }
};

// One stable LSD radix pass over perm (n entries) by digit r: in -> out.
static int rs_pass(HhScratch &sc, hipStream_t st, const uint32_t *in, uint32_t *out, uint32_t n, const RsDigit &r) {
    const uint32_t nblk = (n + kRsBlock - 1) / kRsBlock;
    const uint32_t ngrp = (nblk + kTGrp - 1) / kTGrp;
    uint32_t *hist = sc.rsh, *part = hist + (size_t)nblk * 256, *tot = part + (size_t)ngrp * 256, *total = tot + 256;
    hipLaunchKernelGGL(k_rs_hist, dim3(nblk), dim3(256), 0, st, in, n, r, hist);
    hipLaunchKernelGGL(k_tscan_part, dim3(1, ngrp), dim3(256), 0, st, hist, nblk, 256u, part);
    hipLaunchKernelGGL(k_tscan_mid, dim3(1), dim3(256), 0, st, part, ngrp, 256u, tot);
    hipLaunchKernelGGL(k_tscan_bins, dim3(1), dim3(1024), 0, st, tot, 256u, total);
    hipLaunchKernelGGL(k_tscan_down, dim3(1, ngrp), dim3(256), 0, st, hist, nblk, 256u, part, tot);
    hipLaunchKernelGGL(k_rs_scatter, dim3(nblk), dim3(256), 0, st, in, n, r, hist, tot, total, out);
    GNS_HIP(hipGetLastError());
    return GNS_OK;
}

// Canonical order of n entries of a device list (value desc, flow bytes asc) -> *perm_out
// (a device array of sc's): stable LSD radix passes by (value desc, key bytes 0..3), and by
// the whole key only when two neighbours tie on that.
static int hh_sort(HhScratch &sc, hipStream_t st, const HhSrc &src, uint32_t n, uint32_t **perm_out) {
    const unsigned g = (n + 255) / 256;
    const uint32_t K = src.K;
    GNS_TRY(grow_buf(&sc.u32c, sc.u32c_n, (uint64_t)n * 2));
    const uint32_t nblk = (n + kRsBlock - 1) / kRsBlock, ngrp = (nblk + kTGrp - 1) / kTGrp;
    GNS_TRY(grow_buf(&sc.rsh, sc.rsh_n, (uint64_t)(nblk + ngrp + 1) * 256 + 4));
    uint32_t *tie = sc.rsh + (size_t)(nblk + ngrp + 1) * 256 + 1;
    uint32_t *p[2] = {sc.u32c, sc.u32c + n};
    int cur = 0;
    // LSD: key bytes hi-1..0 (the last first), then the value (least significant byte first,
    // inverted: descending) -> (value desc, key bytes 0..hi-1 asc)
    auto sort_by = [&](uint32_t hi) -> int {
        hipLaunchKernelGGL(k_hh_iota, dim3(g), dim3(256), 0, st, p[0], n);
        cur = 0;
        RsDigit r{1, 0, src};
        for (int b = (int)hi - 1; b >= 0; b--) {
            r.b = (uint32_t)b;
            GNS_TRY(rs_pass(sc, st, p[cur], p[cur ^ 1], n, r));
            cur ^= 1;
        }
        r.mode = 0;
        for (uint32_t b = 0; b < 4; b++) {
            r.b = b;
            GNS_TRY(rs_pass(sc, st, p[cur], p[cur ^ 1], n, r));
            cur ^= 1;
        }
        return GNS_OK;
    };
    HhTrace tr(st);
    GNS_TRY(sort_by(std::min<uint32_t>(K, 4)));
    tr.mark("sort_primary", n);
    if (K > 4) {
        GNS_TRY(small_pin(sc));
        GNS_HIP(hipMemsetAsync(tie, 0, 4, st));
        hipLaunchKernelGGL(k_hh_ties, dim3(g), dim3(256), 0, st, p[cur], n, src, tie);
        GNS_HIP(hipMemcpyAsync(sc.hsm + 4, tie, 4, hipMemcpyDeviceToHost, st));
        GNS_HIP(hipStreamSynchronize(st));
        const uint32_t tflag = sc.hsm[4];
        tr.mark(tflag ? "ties:yes" : "ties:no", n);
        if (tflag) GNS_TRY(sort_by(K));  // the whole key: bytes K-1..0, then the value
        if (tflag) tr.mark("sort_full", n);
    }
    *perm_out = p[cur];
    return GNS_OK;
}

int hh_heavy_list(HhScratch &sc, hipStream_t st, const DictDev &D, uint64_t dict_slots, uint32_t K, uint64_t cells,
                  const uint32_t *val, const uint32_t *fp, uint32_t thr, uint8_t *flows, uint32_t *vals,
                  uint64_t *n_io, uint8_t *rows_dev) {
    HhTrace tr(st);
    GNS_TRY(hh_reserve(sc, cells, dict_slots, K, st));
    GNS_TRY(small_pin(sc));
    tr.mark("reserve", cells);
    // candidate buffer: grows to the number of cells at or above the threshold
    // (no cap: a low threshold can make every bucket a candidate, d*w < 2^32)
    uint32_t nc = 0;
    for (int pass = 0; pass < 2; pass++) {
        // [0] candidates, [1] unique, [2] bad-id flag: zeroed by a kernel on the list's stream
        tr.mark("pre_launch", 0, false);
        hipLaunchKernelGGL(k_fill_u32, dim3(1), dim3(64), 0, st, sc.ncand, (uint64_t)3, 0u);
        tr.mark("launched", 0, false);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_hh_candidates, dim3((unsigned)((cells + 256 * kHhItems - 1) / (256 * kHhItems))), dim3(256), 0,
                               st, val, fp, cells, thr, sc.cand, sc.ncand, (uint32_t)sc.cap);
            e = hipGetLastError();
        }
        tr.mark("cand_kernel", cells);
        if (e == hipSuccess) e = hipMemcpyAsync(sc.hsm, sc.ncand, 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) { set_error("heavy: %s", hipGetErrorString(e)); return GNS_E_HIP; }
        nc = sc.hsm[0];
        tr.mark("candidates", nc);
        if (nc <= sc.cap) break;
        // more candidates than the buffer holds: grow to the count and run again
        dfree(sc.cand);
        sc.cand = nullptr;
        sc.cap = 0;
        const uint64_t want = std::min<uint64_t>(cells, (uint64_t)nc + nc / 8);
        GNS_TRY(dalloc(reinterpret_cast<void **>(&sc.cand), want * 8));
        sc.cap = want;
    }
    const uint64_t *cand = sc.cand;
    // on the device: the max per flow over its buckets, one entry per flow
    uint32_t nu = 0;
    if (nc) {
        const unsigned g = (nc + 255) / 256;
        GNS_TRY(heavy_flow_words(sc, dict_slots, st, true));
        GNS_TRY(grow_buf(&sc.u32a, sc.u32a_n, nc));
        GNS_TRY(grow_buf(&sc.u32b, sc.u32b_n, nc + 1));
        uint32_t *d_nu = sc.ncand + 1, *d_bad = sc.ncand + 2;
        const uint64_t slots = dict_slots;
        hipLaunchKernelGGL(k_hh_best, dim3(g), dim3(256), 0, st, cand, nc, sc.best, sc.hh_epoch, slots, d_bad);
        hipLaunchKernelGGL(k_hh_emit, dim3(g), dim3(256), 0, st, cand, nc, sc.best, sc.mark, sc.hh_epoch, slots,
                           sc.u32a, sc.u32b, d_nu);
        GNS_HIP(hipGetLastError());
        GNS_HIP(hipMemcpyAsync(sc.hsm + 1, d_nu, 8, hipMemcpyDeviceToHost, st));
        GNS_HIP(hipStreamSynchronize(st));
        nu = sc.hsm[1];
        if (sc.hsm[2]) {
            set_error("heavy hitters: a bucket fingerprint names no dictionary slot (corrupt state)");
            return GNS_E_HIP;
        }
        tr.mark("dedupe", nu);
    }
    const uint64_t capn = *n_io;
    *n_io = nu;
    if (nu) {
        const unsigned g = (nu + 255) / 256;
        const uint32_t Kb = K ? K : 1;
        GNS_TRY(grow_buf(&sc.bytes, sc.bytes_n, (uint64_t)nu * Kb));
        GNS_TRY(grow_buf(&sc.obytes, sc.obytes_n, (uint64_t)nu * Kb));
        GNS_TRY(grow_buf(&sc.u32d, sc.u32d_n, (uint64_t)nu));
        tr.mark("grow", nu);
        if (K) hipLaunchKernelGGL(k_ids_to_bytes, dim3(g), dim3(256), 0, st, sc.u32a, (uint64_t)nu, D, sc.bytes);
        tr.mark("ids_to_bytes", nu);
        const HhSrc src{sc.u32b, sc.bytes, K, K};
        uint32_t *perm = nullptr;
        GNS_TRY(hh_sort(sc, st, src, nu, &perm));
        tr.mark("sorted", nu);
        if (rows_dev) {
            if (nu <= capn) {
                hipLaunchKernelGGL(k_hh_gather, dim3(g), dim3(256), 0, st, perm, src, nu, nullptr, nullptr, rows_dev);
                GNS_HIP(hipGetLastError());
                GNS_HIP(hipStreamSynchronize(st));
            }
            return GNS_OK;
        }
        hipLaunchKernelGGL(k_hh_gather, dim3(g), dim3(256), 0, st, perm, src, nu, sc.obytes, sc.u32d, nullptr);
        GNS_HIP(hipGetLastError());
        const uint64_t m = std::min<uint64_t>(nu, capn);
        const uint64_t fb = (flows && K) ? m * K : 0, vb = vals ? m * 4 : 0;
        if (fb + vb > sc.hpin_n) {
            if (sc.hpin) (void)hipHostFree(sc.hpin);
            sc.hpin = nullptr; sc.hpin_n = 0;
            const uint64_t want = 2 * (fb + vb);
            GNS_HIP(hipHostMalloc(reinterpret_cast<void **>(&sc.hpin), want, hipHostMallocDefault));
            sc.hpin_n = want;
        }
        if (fb) GNS_HIP(hipMemcpyAsync(sc.hpin, sc.obytes, fb, hipMemcpyDeviceToHost, st));
        if (vb) GNS_HIP(hipMemcpyAsync(sc.hpin + fb, sc.u32d, vb, hipMemcpyDeviceToHost, st));
        GNS_HIP(hipStreamSynchronize(st));
        tr.mark("gather_d2h", m);
        if (fb) memcpy(flows, sc.hpin, fb);
        if (vb) memcpy(vals, sc.hpin + fb, vb);
        tr.mark("host_copy", m);
    }
    return GNS_OK;
}

// gns_hh_order_rows' order for a caller that owns its scratch and its stream: nothing is
// copied to the host and the stream is left running (the caller synchronizes it).  Keys
// longer than four bytes cost one small read-back inside the order (the tie flag).
int hh_order_rows_dev(HhScratch &sc, hipStream_t st, const uint8_t *rows, uint32_t K, uint32_t n, uint8_t *out_rows) {
    if (n == 0) return GNS_OK;
    const HhSrc src{nullptr, rows, K, K + 4};
    uint32_t *perm = nullptr;
    GNS_TRY(hh_sort(sc, st, src, n, &perm));
    hipLaunchKernelGGL(k_hh_gather, dim3((n + 255) / 256), dim3(256), 0, st, perm, src, n, nullptr, nullptr, out_rows);
    GNS_HIP(hipGetLastError());
    return GNS_OK;
}

}  // namespace gns

using namespace gns;

extern "C" {

// per device, per host thread: the sort scratch of gns_hh_order_rows (grow-only; it lives as long
// as the thread -- freeing device memory from a thread-exit destructor could run after the HIP
// runtime's own teardown at process exit)
static thread_local std::vector<HhScratch *> t_hh_scratch;

int gns_hh_order_rows(const uint8_t *rows, uint32_t key_bytes, uint64_t n, uint8_t *out_rows, int device) {
    if ((n && (!rows || !out_rows)) || key_bytes > 37) { set_error("bad argument"); return GNS_E_ARG; }
    if (n >= (1ull << 31)) { set_error("%llu rows (max 2^31 - 1)", (unsigned long long)n); return GNS_E_RANGE; }
    if (n == 0) return GNS_OK;
    (void)hipGetLastError();
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        (void)hipGetLastError(); set_error("device %d not available", device); return GNS_E_NODEV;
    }
    GNS_HIP(hipSetDevice(device));
    if ((int)t_hh_scratch.size() <= device) t_hh_scratch.resize(device + 1, nullptr);
    if (!t_hh_scratch[device]) t_hh_scratch[device] = new HhScratch();
    HhScratch &sc = *t_hh_scratch[device];
    hipStream_t st = nullptr;  // the legacy stream: ordered after the caller's device writes
    const HhSrc src{nullptr, rows, key_bytes, key_bytes + 4};
    uint32_t *perm = nullptr;
    GNS_TRY(hh_sort(sc, st, src, (uint32_t)n, &perm));
    hipLaunchKernelGGL(k_hh_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, perm, src, (uint32_t)n,
                       nullptr, nullptr, out_rows);
    GNS_HIP(hipGetLastError());
    GNS_HIP(hipStreamSynchronize(st));
    return GNS_OK;
}

}  // extern "C"
